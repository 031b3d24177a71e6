// svt_evidence.inc -- per-breakpoint evidence of refined calls (include/svtrek_evidence.h; included
// by svt_engine.hip after the refine kernels).
//
// For a breakpoint refined to R the record is {support, depth, lo, hi}: support = the window's
// candidates c with |c - R| <= ci, lo / hi their smallest / largest, depth = reads with
// pos <= R < endpos.  One wave per breakpoint (window g < n: locus g's first, n + i: locus i's
// second, as the refine kernels number them); everything a wave branches on is wave-uniform.
//   support, bucket path (bk_eligible == 1): the value-bucketed index files every event by the
//     value it votes with, so the supporting events sit in the one or two 1 kb buckets covering
//     [R - ci, R + ci]; each is tested against the WINDOW (bk_cand) and against R.
//   support, exact fallback (every other window: SVTREK_INDEX=lists, band off, bk_eligible == 0):
//     the span walk's events of the window's reads (span_query + span_cand) through the same test.
//   support, per-read walk (e >= WEXACT, and the sentinel windows below): the reference's own
//     uint32 walk (gather_perread) into the counting sink.
//   depth: the region query [R, R + 1) (read_range), then endpos > R counted over its range.
// The sentinel: no event carries the value of a refine_end leading-S read whose walk breaks past
// e (the position after the break op + 1 >= e + 2; v.w is the read's full walk end).  The bucket
// and span paths vote it as e + 2 (KParams::sent_ok), which is exact for the vote but not for a
// support radius that reaches e + 2: a refine_end window with R + ci >= e + 2 takes the per-read
// walk.  (Not at the default parameters: R < imp + range, so R + ci < e + 2 whenever
// narrow + 2 >= range + ci.)
// Candidates and R compare as the reference's int values, differences in 64 bits.

// The counting sink: per lane the supporting candidates it saw (ev_reduce sums the lanes).
struct EvSink {
    int32_t r, ci;   // R, consensus_interval (>= 0)
    uint32_t n = 0;
    int32_t mn = INT32_MAX, mx = INT32_MIN;
    __device__ __forceinline__ void push(bool pred, int32_t val) {
        const int64_t d = (int64_t)val - (int64_t)r;
        const bool h = pred && (d < 0 ? -d : d) <= (int64_t)ci;
        n += h ? 1u : 0u;
        mn = h ? min(mn, val) : mn;
        mx = h ? max(mx, val) : mx;
    }
};

__device__ __forceinline__ void ev_reduce(EvSink &sk) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        sk.n += __shfl_xor(sk.n, d, WAVE);
        sk.mn = min(sk.mn, __shfl_xor(sk.mn, d, WAVE));
        sk.mx = max(sk.mx, __shfl_xor(sk.mx, d, WAVE));
    }
}

// Bucket path: the events of the buckets covering [R - ci, R + ci] (0 <= R < 2^30, ci <= LV_WMAX).
template <int KIND>
__device__ __forceinline__ void ev_bucket(const BkIndex &B, int tid, const BkWin &W, EvSink &sk) {
    const int ln = lane_id();
    uint32_t E0, E1;
    bk_range(B, bk_array(KIND), tid, max<int64_t>((int64_t)sk.r - sk.ci, 0), (int64_t)sk.r + sk.ci, E0, E1);
    for (uint32_t b = E0; b < E1; b += WAVE) {
        const uint32_t i = b + (uint32_t)ln;
        const uint4 v = i < E1 ? B.ev[i] : make_uint4(0, 0, 0, 0);
        uint32_t val = 0;
        const int c = i < E1 ? bk_cand<KIND>(v, W, val) : 0;   // c == 2: a value >= e + 2 > R + ci (the caller's test)
        sk.push(c == 1, (int32_t)val);
    }
}

// Span path: the events of the window's reads (e < WEXACT); SPAN_U loads in flight per lane.
template <int KIND>
__device__ __forceinline__ void ev_span(const DevPileup &P, int tid, uint32_t s, uint32_t e, EvSink &sk) {
    const int64_t beg = (int64_t)(uint32_t)(s - 1u), end = (int64_t)(uint32_t)(e - 1u);
    uint64_t E0, E1;
    if (!span_query<KIND>(P, tid, beg, end, E0, E1)) return;
    const int32_t beg32 = (int32_t)(uint32_t)(s - 1u);
    const int ln = lane_id();
    const uint4 *ev = KIND == K_INS ? P.spI : P.spD;
    for (uint64_t b = E0; b < E1; b += SPAN_U * WAVE) {
        uint4 v[SPAN_U];
#pragma unroll
        for (int u = 0; u < SPAN_U; u++) {
            const uint64_t j = b + (uint64_t)(u * WAVE + ln);
            v[u] = j < E1 ? ev[j] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < SPAN_U; u++) {
            const uint64_t j = b + (uint64_t)(u * WAVE + ln);
            uint32_t val = 0;
            const bool c = j < E1 && span_cand<KIND>(v[u], s, e, beg32, val);   // a stop past e: e + 2 > R + ci
            sk.push(c, (int32_t)val);
        }
    }
}

template <int KIND>
__device__ __forceinline__ void ev_support(const KArgs &a, int chrom, uint32_t s, uint32_t e, uint32_t imp, EvSink &sk) {
    const bool sentinel = KIND == K_END && (int64_t)sk.r + (int64_t)sk.ci >= (int64_t)e + 2;
    if (e >= WEXACT || sentinel) {
        WinStats st;
        gather_perread<KIND, false>(a.pile, chrom - 1, s, e, sk, st);
        return;
    }
    BkWin W;
    const int el = bk_eligible(a, KIND, chrom, s, e, imp, W);
    if (el < 0) return;   // no reads (A3)
    if (el == 1 && sk.r >= 0 && sk.r < (1 << 30)) ev_bucket<KIND>(a.bk, chrom - 1, W, sk);
    else ev_span<KIND>(a.pile, chrom - 1, s, e, sk);
}

// Reads of contig tid with pos <= a and endpos > b (a, b >= 0): the region query [b, max(a, b) + 1) yields
// every read with pos <= max(a, b) that ends past b, then both bounds are tested, 64 reads a trip.
__device__ __forceinline__ uint32_t span_reads(const DevPileup &P, int tid, int64_t a, int64_t b) {
    int64_t lo, hi;
    if (!read_range(P, tid, b, max(a, b) + 1, lo, hi)) return 0u;
    const int ln = lane_id();
    uint32_t cnt = 0;
    for (int64_t base = lo; base < hi; base += WAVE) {
        const int64_t r = base + ln;
        const uint2 pe = r < hi ? *reinterpret_cast<const uint2 *>(P.rec + r) : make_uint2(0u, 0u);   // {pos, endpos}
        cnt += (uint32_t)__popcll(ballot(r < hi && (int64_t)(int32_t)pe.x <= a && (int64_t)(int32_t)pe.y > b));
    }
    return cnt;
}

// Reads of contig tid with pos <= R < endpos.
__device__ __forceinline__ uint32_t ev_depth(const DevPileup &P, int tid, uint32_t R) {
    return span_reads(P, tid, (int64_t)R, (int64_t)R);
}

__global__ __launch_bounds__(64 * WPB) void evidence_kernel(KArgs a, const svt_result *refined, svt_evidence *out) {
    const uint32_t g = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (g >= 2 * a.n) return;
    uint32_t li, w, s = 0, e = 0, imp = 0;
    int32_t chrom;
    const int kind = window_of(a, g, li, w, chrom, s, e, imp);
    const uint32_t R = (uint32_t)uniform_i((int32_t)reinterpret_cast<const uint32_t *>(refined)[2 * (size_t)li + w]);
    uint4 rec = make_uint4(0u, 0u, SVT_NA, SVT_NA);
    if (R != SVT_NA) {
        EvSink sk{(int32_t)R, a.prm.ci};
        if (a.prm.ci >= 0) {
            if (kind == K_INS) ev_support<K_INS>(a, chrom, s, e, imp, sk);
            else if (kind == K_START) ev_support<K_START>(a, chrom, s, e, imp, sk);
            else if (kind == K_END) ev_support<K_END>(a, chrom, s, e, imp, sk);
        }
        ev_reduce(sk);
        rec.x = sk.n;
        rec.y = ev_depth(a.pile, chrom - 1, R);
        if (sk.n) { rec.z = (uint32_t)sk.mn; rec.w = (uint32_t)sk.mx; }
    }
    // lanes 0-3 store one word each (one 16-B vector store; svt_evidence is only 4-B aligned)
    const int ln = lane_id();
    const uint32_t word = ln == 0 ? rec.x : ln == 1 ? rec.y : ln == 2 ? rec.z : rec.w;
    if (ln < 4) reinterpret_cast<uint32_t *>(out + 2 * (size_t)li + w)[ln] = word;
}
