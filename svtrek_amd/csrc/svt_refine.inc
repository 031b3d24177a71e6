// svt_refine.inc -- the wave-per-window refine path (included by svt_engine.hip after svt_bucket.inc):
// refine_kernel / refine_span_kernel (refine_body), refine_redo_kernel for the lane kernel's
// left-overs, and the sliding_window_ins kernels.

// One wave per query window, WPB independent waves per workgroup.  Window g < n is locus
// g's first window (DEL: refine_start over [pos-wider, pos+narrow], INS: refine_ins),
// window n + i is locus i's second (DEL: refine_end over end +- narrow): the wide windows
// are dispatched first, so the short ones fill the tail.
// (Workgroups in dispatch order: an XCD-aware swizzle -- each XCD a contiguous run of
// neighbouring loci -- measured slower, 37.1 vs 35.3 us on cfg2: the launch's records stay in
// the MALL across launches, so L2 locality buys nothing.)
constexpr int WPB = 4;

// The refine kernels are held to 64 VGPRs = 8 waves per SIMD (the CU's maximum): their walks
// are bound by dependent-load latency, so resident waves are what hide it.
constexpr int REFINE_WAVES = 8;
#define SVT_WAVES(n) __attribute__((amdgpu_waves_per_eu(n, n)))

template <bool COUNT>
__device__ __forceinline__ void refine_body(const KArgs &a);

template <bool COUNT>
__global__ __launch_bounds__(64 * WPB) void refine_kernel(KArgs a) { refine_body<COUNT>(a); }

__global__ __launch_bounds__(64 * WPB) SVT_WAVES(REFINE_WAVES) void refine_span_kernel(KArgs a) { refine_body<false>(a); }

__device__ __forceinline__ void write_result(const KArgs &a, uint32_t li, uint32_t w, uint32_t r) {
    if (a.rec_out) {   // gather record {index, start, end, 0} (SURVEY.md §8(e))
        uint32_t *o = reinterpret_cast<uint32_t *>(a.rec_out + li);
        o[1 + w] = r;
        if (w == 0) {
            o[0] = a.rec_index ? a.rec_index[li] : a.rec_base + li;
            o[3] = 0u;
        }
    } else {
        uint32_t *o = reinterpret_cast<uint32_t *>(a.out + li);
        o[w] = r;
    }
}

// A2 (audit.c:176-225) for window g: kind (-1: none -> NA), s, e, pos of the vote.
__device__ __forceinline__ int window_of(const KArgs &a, uint32_t g, uint32_t &li, uint32_t &w, int32_t &chrom,
                                         uint32_t &s, uint32_t &e, uint32_t &imp) {
    w = g >= a.n ? 1u : 0u;
    li = g - w * a.n;
    const svt_locus L = a.loci[li];
    const int32_t type = uniform_i(L.type);
    chrom = uniform_i(L.chrom);
    const uint32_t pos = (uint32_t)uniform_i((int32_t)L.pos), end = (uint32_t)uniform_i((int32_t)L.end);
    const KParams &k = a.prm;
    // INV: refine_point collects only when sv_type == SV_INS (refinement.c:250): NA, NA
    if (type == T_INS && w == 0) { s = pos - (uint32_t)k.median; e = pos + (uint32_t)k.median; imp = pos; return K_INS; }
    if (type == T_DEL) {
        if (w == 0) { s = pos - (uint32_t)k.wider; e = pos + (uint32_t)k.narrow; imp = pos; return K_START; }
        s = end - (uint32_t)k.narrow; e = end + (uint32_t)k.narrow; imp = end;
        return K_END;
    }
    return -1;
}

// The gather of one window kind (+ the COUNT builds' work counters); the candidates are
// left in lds.cand, their count is returned.
template <int KIND, bool COUNT>
__device__ __forceinline__ int32_t gather_window(const KArgs &a, WinLds &lds, int chrom, uint32_t s, uint32_t e,
                                                 unsigned long long *wk) {
    WinStats st;
    Sink sink{lds.cand, CAP, &lds.ncand};
    const int32_t n = gather<KIND, COUNT>(a, chrom - 1, s, e, sink, st);
    if (COUNT && lane_id() == 0) {
        wk[W_WINDOWS] += 1; wk[W_READS] += st.reads; wk[W_OPS] += st.ops; wk[W_CANDS] += (unsigned long long)n;
        wk[W_QUERIES] += st.queries; wk[W_PROBE] += st.probe; wk[W_RANGE] += st.range; wk[W_LREADS] += st.lreads;
        wk[W_LENTRIES] += st.lentries; wk[W_STOPS] += st.stops; wk[W_STOPCH] += st.stopch;
        wk[W_SQUERIES] += st.squeries; wk[W_SPAN] += st.span;
    }
    return n;
}

// One window wave-wide: its gather, then its vote.
template <int KIND, bool COUNT, int VOTE = V_CONSENSUS>
__device__ __forceinline__ int32_t refine_window(const KArgs &a, WinLds &lds, int chrom, uint32_t s, uint32_t e, uint32_t imprecise,
                                 unsigned long long *wk, int32_t &support) {
    const int32_t n = gather_window<KIND, COUNT>(a, lds, chrom, s, e, wk);
    return vote_window<KIND, COUNT, VOTE>(a, lds, chrom, s, e, imprecise, n, wk, support);
}

template <bool COUNT>
__device__ __forceinline__ void refine_body(const KArgs &a) {
    __shared__ WinLds lds_all[WPB];
    const uint32_t wid = threadIdx.x >> 6;
    const uint32_t g = blockIdx.x * WPB + wid;
    if (g >= 2 * a.n) return;
    WinLds &lds = lds_all[wid];
    const uint32_t w = g >= a.n ? 1u : 0u, li = g - w * a.n;
    const svt_locus L = a.loci[li];
    const int32_t type = uniform_i(L.type), chrom = uniform_i(L.chrom);
    const uint32_t pos = (uint32_t)uniform_i((int32_t)L.pos), end = (uint32_t)uniform_i((int32_t)L.end);
    unsigned long long wk[W_N] = {};
    const KParams &k = a.prm;
    // A2 (audit.c:176-225): the window of this wave.  INV: refine_point collects only when
    // sv_type == SV_INS (refinement.c:250), so both windows vote on 0 candidates -> -1 for
    // every min_count >= 1 (validated): NA, NA.
    int kind = -1;
    uint32_t s = 0, e = 0, imp = 0;
    if (type == T_INS && w == 0) {
        kind = K_INS; s = pos - (uint32_t)k.median; e = pos + (uint32_t)k.median; imp = pos;
    } else if (type == T_DEL) {
        if (w == 0) { kind = K_START; s = pos - (uint32_t)k.wider; e = pos + (uint32_t)k.narrow; imp = pos; }
        else { kind = K_END; s = end - (uint32_t)k.narrow; e = end + (uint32_t)k.narrow; imp = end; }
    }
    uint32_t r = SVT_NA;
    // the value buckets first (svt_bucket.inc); the span lists for the windows they do not take
    const bool bk_done = !COUNT && kind >= 0 && refine_any_bk<false>(a, lds, kind, chrom, s, e, imp, wk, r);
    if (kind >= 0 && !bk_done) {
        // the kind-specific gathers, then ONE copy of the sort + vote for all kinds (code size:
        // the three inlined copies of the vote no longer compete for the instruction cache)
        int32_t n;
        if (kind == K_INS) n = gather_window<K_INS, COUNT>(a, lds, chrom, s, e, wk);
        else if (kind == K_START) n = gather_window<K_START, COUNT>(a, lds, chrom, s, e, wk);
        else n = gather_window<K_END, COUNT>(a, lds, chrom, s, e, wk);
        n = uniform_i(n);
        int32_t sup = 0;
        if (n < k.min_count) r = SVT_NA;                    // refinement.c:43-45
        else if (n <= CAP) r = (uint32_t)sort_and_vote<V_CONSENSUS>(lds.cand, lds.pre, n, (int32_t)imp, k, sup);
        else if (kind == K_INS) r = (uint32_t)vote_window<K_INS, COUNT, V_CONSENSUS>(a, lds, chrom, s, e, imp, n, wk, sup);
        else if (kind == K_START) r = (uint32_t)vote_window<K_START, COUNT, V_CONSENSUS>(a, lds, chrom, s, e, imp, n, wk, sup);
        else r = (uint32_t)vote_window<K_END, COUNT, V_CONSENSUS>(a, lds, chrom, s, e, imp, n, wk, sup);
        if (COUNT) {   // what the bucket path reads for this window (its result is the same)
            wave_sync();
            uint32_t rb = 0;
            (void)refine_any_bk<true>(a, lds, kind, chrom, s, e, imp, wk, rb);
        }
    }
    if (lane_id() == 0) {
        write_result(a, li, w, r);
        if (COUNT)
            for (int i = 0; i < W_N; i++)
                if (wk[i]) atomicAdd(a.work + i, wk[i]);
    }
}

// The lane kernel's left-over windows (band off, > LV_CAP band elements, > CAP candidates,
// slow reads, windows ending at or past 2^31), one wave each, re-gathered and voted
// wave-wide (refine_window); the grid strides over the list.  Also resets the counter the
// next launch will use.
__global__ __launch_bounds__(64 * WPB) SVT_WAVES(REFINE_WAVES) void refine_redo_kernel(KArgs a) {
    __shared__ WinLds lds_all[WPB];
    const uint32_t wid = threadIdx.x >> 6;
    const uint32_t gw = blockIdx.x * WPB + wid, nwv = gridDim.x * WPB;
    if (gw == 0 && lane_id() == 0) *a.redo_next = 0u;
    const uint32_t cnt = (uint32_t)uniform_i((int32_t)__hip_atomic_load(a.redo_ctr, __ATOMIC_RELAXED,
                                                                         __HIP_MEMORY_SCOPE_AGENT));
    WinLds &lds = lds_all[wid];
    for (uint32_t idx = gw; idx < cnt; idx += nwv) {
        const uint32_t g = (uint32_t)uniform_i((int32_t)a.redo_list[idx]);
        uint32_t li, w, s = 0, e = 0, imp = 0;
        int32_t chrom;
        const int kind = window_of(a, g, li, w, chrom, s, e, imp);
        unsigned long long wk[W_N];
        int32_t sup;
        uint32_t r = SVT_NA;
        if (kind >= 0 && refine_any_bk<false>(a, lds, kind, chrom, s, e, imp, wk, r)) {}   // the value buckets
        else if (kind == K_INS) r = (uint32_t)refine_window<K_INS, false>(a, lds, chrom, s, e, imp, wk, sup);
        else if (kind == K_START) r = (uint32_t)refine_window<K_START, false>(a, lds, chrom, s, e, imp, wk, sup);
        else if (kind == K_END) r = (uint32_t)refine_window<K_END, false>(a, lds, chrom, s, e, imp, wk, sup);
        if (lane_id() == 0) write_result(a, li, w, r);
        wave_sync();
    }
}

// sliding_window_ins mode (sliding_window.c:8-97): one wave per sub-window.  A sub-window
// is refine_ins's window exactly -- the same region query (sub_start-1, sub_end-1, :27),
// the same walk (I >= 50 collects rp, advance unless I/S, break when rp > sub_end,
// :30-54) -- so it reuses the span gather; only the vote differs (sw_vote).
__global__ __launch_bounds__(64 * WPB) void sw_kernel(KArgs a) {
    __shared__ WinLds lds_all[WPB];
    const uint32_t wid = threadIdx.x >> 6;
    const uint32_t g = blockIdx.x * WPB + wid;
    if (g >= a.n) return;
    const uint4 q = a.sw_sub[g];
    const int32_t chrom = uniform_i((int32_t)q.x);
    const uint32_t s = (uint32_t)uniform_i((int32_t)q.y), e = (uint32_t)uniform_i((int32_t)q.z);
    unsigned long long wk[W_N];
    int32_t sup = 0;
    const int32_t c = refine_window<K_INS, false, V_SLIDING>(a, lds_all[wid], chrom, s, e, 0u, wk, sup);
    if (lane_id() == 0) a.sw_out[g] = make_int2(c, sup);
}

// bestCandidateOverall per query over its sub-windows in order (sliding_window.c:86-92).
__global__ void sw_reduce_kernel(const int2 *sub, const uint64_t *off, uint32_t nq, int32_t *best) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    int32_t b = -1, m = 0;
    for (uint64_t k = off[q]; k < off[q + 1]; k++) {
        const int2 v = sub[k];
        if (v.x != -1 && v.y > m) { m = v.y; b = v.x; }
    }
    best[q] = b;
}
