// svt_bucket.inc -- the value-bucketed event index, refine side (included by svt_engine.hip between
// svt_vote.inc and svt_refine.inc; the build kernels are in svt_bucket_build.inc).
//
// Why (VERDICT r05, item 1): a window's candidates that matter to consensus_pos
// (refinement.c:41-101) are its exact band -- values in (pos - w, pos + w), w = range + max(ci, 0)
// -- plus three facts of the whole multiset: some candidate at or below the band (BELOW), some at
// or above it (ABOVE), and its minimum when that lies in the band (band_filter, Band).  The span
// walk of rounds 1-5 found them by walking every event of every read the window's region query
// yields (~126 events per cfg4 window, each event walked ~8.7 times per step by overlapping
// windows).  Here every candidate event is filed ONCE per rebuild by the value it would vote with,
// in 1 kb buckets per contig, one array per window kind:
//   S  (refine_start, refinement.c:124/:147): D > 50 events and trailing-S markers, by walk position x;
//   E  (refine_end, :188-221): D > 50 events by x + len + 1, leading-S markers by walk end + 1;
//   I  (refine_ins, :299): I >= 50 events by x;
//   L  (refine_end's leading-S stops): the leading-S markers again, by read start.
// Events are self-contained ({x, CIGAR word, endpos, read pos} -- {pos, SP_LEAD, endpos, walk end}
// for the leading-S markers), so every test of the reference's walk and of htslib's region query
// is a test of the event: pos < query end, endpos > query beg (hts_itr_next), x <= e (the op is
// reached before the walk breaks, refinement.c:141-145), s <= x (trailing S), s <= pos (leading S).
// A window then reads
//   * its band: the events of the buckets covering (lo, hi) -- ~20 on cfg4, one slot of a wave;
//   * BELOW: one prefix maximum per bucket of a key that is > beg exactly when an event at or below
//     the bucket's end is a candidate below the band -- for every value <= lo the window's other
//     tests hold by themselves (lo < query end: pos_r <= x <= lo; x <= e), so the key is the one
//     test left: endpos (D, I), min(x, endpos) (trailing S: s <= x is x > beg), read pos (leading
//     S: s <= pos; endpos > pos > beg follows);
//   * ABOVE, only when the vote reads it (no candidate below pos - 25: lane_vote's right pass
//     start, refinement.c:78): the bounded walks [hi, e] (S, I: every candidate is <= e), and for
//     refine_end [hi, e + 1], then the leading-S reads starting in [s, e - 2] whose walk passes e
//     (L) and the D ops spanning e (S, from e - longest D > 50 of the contig).
// The per-window work is a fixed number of table reads plus the band's events; exactness is the
// oracle's (tests/test_gpu_parity.py, tests/test_gpu_lane_wide.py, tests/test_bucket_model.py), the
// design was checked against the oracle on cfg2/cfg3/cfg4 and fuzzed pileups before this code
// existed (DESIGN.md "Value buckets").
__device__ __forceinline__ int bk_array(int kind) { return kind == K_START ? BA_S : kind == K_END ? BA_E : BA_I; }

// Window [s, e] of a lane-path kind, its band (lo, hi) = (imp - w, imp + w).
struct BkWin {
    uint32_t s, e;
    int32_t beg;                  // s - 1 (< 2^30: windows reaching the buckets end below WEXACT)
    int32_t lo, hi;
};

// The bucket range of values [v0, v1] (v0 <= v1, both >= 0) of array A in contig tid: events [E0, E1).
__device__ __forceinline__ void bk_range(const BkIndex &B, int A, int tid, int64_t v0, int64_t v1, uint32_t &E0,
                                         uint32_t &E1) {
    const uint32_t nb = B.cnb[tid];
    const uint64_t base = B.cbase[tid];
    const uint64_t b0 = (uint64_t)min<int64_t>(v0 >> BKS, (int64_t)nb - 1), b1 = (uint64_t)min<int64_t>(v1 >> BKS, (int64_t)nb - 1);
    const uint32_t *off = B.off + (uint64_t)A * (B.nbk + 1);
    E0 = off[base + b0];
    E1 = off[base + b1 + 1];
}

// One event's verdict for window W of kind KIND: 0 not a candidate, 1 a candidate with value val,
// 2 a refine_end leading-S read whose walk passes e (a value >= e + 2 >= hi: KParams::sent_ok).
template <int KIND>
__device__ __forceinline__ int bk_cand(const uint4 &v, const BkWin &W, uint32_t &val) {
    const uint32_t op = v.y & 0xfu;
    const bool ovl = (int32_t)v.z > W.beg;                  // hts_itr_next: endpos > beg
    if (KIND == K_END && op == SP_LEAD) {                   // refinement.c:210-220; v.x = pos, v.w = walk end
        const bool lead = ovl && v.x >= W.s && v.x + 2u <= W.e;   // s <= pos, pos < query end (= e - 1)
        val = v.w + 1u;
        return !lead ? 0 : v.w > W.e ? 2 : 1;
    }
    const bool y = ovl && v.w + 2u <= W.e && v.x <= W.e;   // yielded (pos < e - 1), reached (x <= e)
    val = KIND == K_END ? v.x + (v.y >> 4) + 1u : v.x;      // :198 / :134, :158, :309
    if (KIND == K_START) return y && (op == OP_DEL || (op == SP_TRAIL && v.x >= W.s));
    if (KIND == K_END) return y && op == OP_DEL;
    return y && op == OP_INS;
}

// Phase 0 of the lane kernel (and the wave-wide path) for one window: its band's events and the
// BELOW fact from the prefix maxima.  False: the window has no reads (A3) -- nb = 0.
__device__ __forceinline__ bool bk_query(const BkIndex &B, int kind, int tid, const BkWin &W, uint32_t &E0,
                                         uint32_t &E1, bool &below) {
    E0 = E1 = 0;
    below = false;
    const int A = bk_array(kind);
    const uint32_t nb = B.cnb[tid];
    const uint64_t base = B.cbase[tid];
    const int64_t lo = W.lo, hi = W.hi;   // hi - 1 >= 0 (imp >= 0, w >= 26)
    const uint64_t bl = lo < 0 ? 0ull : (uint64_t)min<int64_t>(lo >> BKS, (int64_t)nb - 1);
    const uint64_t bh = (uint64_t)min<int64_t>((hi - 1) >> BKS, (int64_t)nb - 1);
    const uint32_t *off = B.off + (uint64_t)A * (B.nbk + 1);
    E0 = off[base + bl];
    E1 = off[base + bh + 1];
    if (bl > 0) below = B.pm[(uint64_t)A * (B.nbk + 1) + base + bl - 1] > W.beg;
    return true;
}

// Does the lane path (and the wave-wide bucket path) take window [s, e] of kind KIND?  The
// conditions of lane_query (band on, e < WEXACT, |imp| < 2^30, refine_end's sent_ok, lo >= -2^29)
// plus lo < query end (every value <= lo then passes the window's other tests: see the prefix
// maxima above).  -1: no reads at all (NA); 0: the span-list path; 1: the buckets.
__device__ __forceinline__ int bk_eligible(const KArgs &a, int kind, int chrom, uint32_t s, uint32_t e, uint32_t imp,
                                           BkWin &W) {
    const KParams &k = a.prm;
    const int32_t bw = k.range + max(k.ci, 0);
    constexpr int32_t LIM = 1 << 30;
    const bool band_ok = k.range > SV_MIN_LENGTH / 2 && bw <= LV_WMAX && k.ci >= -LV_WMAX;
    if (!a.bk.on || e >= WEXACT || (kind == K_END && !k.sent_ok) || !band_ok || (int32_t)imp <= -LIM ||
        (int32_t)imp >= LIM)
        return 0;
    const int32_t lo = (int32_t)imp - bw;
    if (lo < -(1 << 29)) return 0;
    const int tid = chrom - 1;
    const int64_t beg = (int64_t)(uint32_t)(s - 1u), qend = (int64_t)(uint32_t)(e - 1u);
    if (tid < 0 || tid >= a.pile.n_targets || qend <= beg) return -1;   // A3: no reads
    if (a.pile.tid_off[tid + 1] == a.pile.tid_off[tid]) return -1;
    if ((int64_t)lo >= qend) return 0;
    W.s = s;
    W.e = e;
    W.beg = (int32_t)beg;
    W.lo = lo;
    W.hi = (int32_t)imp + bw;
    return 1;
}

// ---- the wave-wide bucket path: one window per wave (refine_span_kernel below 64K windows,
// refine_redo_kernel for the lane kernel's left-overs -- bands of more than LV_CAP members, ABOVE
// pending -- and the counting kernel).  Returns consensus_pos's result, or BK_FALLBACK when the
// band holds more than CAP members (the span-list path with its spill slabs then votes it).
constexpr int32_t BK_FALLBACK = INT32_MIN;

// Any event of [E0, E1) passing pred (64 a step; the steps stop at the first hit).
template <typename Pred>
__device__ __forceinline__ bool bk_any(const uint4 *ev, uint32_t E0, uint32_t E1, Pred pred, unsigned long long &walked) {
    const int ln = lane_id();
    for (uint32_t b = E0; b < E1; b += WAVE) {
        const uint32_t i = b + (uint32_t)ln;
        const uint4 v = i < E1 ? ev[i] : make_uint4(0, 0, 0, 0);
        walked += min(E1 - b, (uint32_t)WAVE);
        if (ballot(i < E1 && pred(v))) return true;
    }
    return false;
}

// ABOVE of window W when the vote needs it (see the file comment): bounded walks only.
template <int KIND>
__device__ __forceinline__ bool bk_above(const BkIndex &B, int tid, const BkWin &W, unsigned long long &walked) {
    uint32_t E0, E1;
    const int A = bk_array(KIND);
    const int64_t top = KIND == K_END ? (int64_t)W.e + 1 : (int64_t)W.e;   // every non-breaking candidate is <= top
    if ((int64_t)W.hi <= top) {
        bk_range(B, A, tid, W.hi, top, E0, E1);
        if (bk_any(B.ev, E0, E1, [&](const uint4 &v) {
                uint32_t val;
                const int c = bk_cand<KIND>(v, W, val);
                return c == 2 || (c == 1 && (int32_t)val >= W.hi);
            }, walked))
            return true;
    }
    if (KIND != K_END) return false;
    // leading-S reads starting in [s, e - 2] (yielded) whose walk passes e: values >= e + 2
    if (W.e >= W.s + 2u) {
        bk_range(B, BA_L, tid, W.s, (int64_t)W.e - 2, E0, E1);
        if (bk_any(B.ev, E0, E1, [&](const uint4 &v) {
                uint32_t val;
                return bk_cand<K_END>(v, W, val) == 2;
            }, walked))
            return true;
    }
    // D > 50 ops reached before e that end past it (x <= e < x + len: value x + len + 1 > e + 1)
    const uint32_t md = B.maxd[tid];
    if (md == 0u) return false;
    bk_range(B, BA_S, tid, max<int64_t>((int64_t)W.e - (int64_t)md, 0), W.e, E0, E1);
    return bk_any(B.ev, E0, E1, [&](const uint4 &v) {
        uint32_t val;
        return (v.y & 0xfu) == OP_DEL && bk_cand<K_END>(v, W, val) == 1 && val > W.e + 1u;
    }, walked);
}

// The window's band into lds.cand (wave-wide), its facts, then sort + vote (sort_and_vote with the
// band given: Band's counts from the members and the two facts).
template <int KIND, bool COUNT>
__device__ __forceinline__ int32_t refine_window_bk(const KArgs &a, WinLds &lds, int tid, const BkWin &W, uint32_t imp,
                                                    unsigned long long *wk) {
    const BkIndex &B = a.bk;
    const KParams &k = a.prm;
    const int ln = lane_id();
    uint32_t E0, E1;
    bool below;
    bk_query(B, KIND, tid, W, E0, E1, below);
    const uint4 *ev = B.ev;
    unsigned long long walked = E1 - E0;
    int32_t cnt = 0, mn = INT32_MAX;
    bool above = false;
    for (uint32_t b = E0; b < E1; b += SPAN_U * WAVE) {
        uint4 v[SPAN_U];
        const uint32_t left = E1 - b;
#pragma unroll
        for (int u = 0; u < SPAN_U; u++) {
            const uint32_t j = b + (uint32_t)(u * WAVE + ln);
            v[u] = (uint32_t)(u * WAVE + ln) < left ? ev[j] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < SPAN_U; u++) {
            if ((uint32_t)(u * WAVE) >= left) break;
            uint32_t val = 0;
            const int c = (uint32_t)(u * WAVE + ln) < left ? bk_cand<KIND>(v[u], W, val) : 0;
            const int32_t x = (int32_t)val;
            const bool mem = c == 1 && x > W.lo && x < W.hi;
            below |= ballot(c == 1 && x <= W.lo) != 0ull;
            above |= ballot(c == 2 || (c == 1 && x >= W.hi)) != 0ull;
            const uint64_t m = ballot(mem);
            const int32_t idx = cnt + (int32_t)mbcnt(m);
            if (mem && idx < CAP) lds.cand[idx] = x;
            if (mem) mn = min(mn, x);
            cnt += (int32_t)__popcll(m);
        }
    }
    if (COUNT && ln == 0) { wk[W_BQ] += 1; wk[W_BEV] += walked; }
    if (cnt < k.min_count) return -1;                       // refinement.c:43-45 (see LaneBand)
    if (cnt > CAP) return BK_FALLBACK;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) mn = min(mn, __shfl_xor(mn, d, WAVE));
    const int32_t pos = (int32_t)imp;
    const bool lt = below || mn < pos - SV_MIN_LENGTH / 2;
    if (!lt && !above) {                                    // the right pass starts at the maximum
        unsigned long long w2 = 0;
        above = bk_above<KIND>(B, tid, W, w2);
        if (COUNT && ln == 0) wk[W_BEV] += w2;
    }
    wave_sync();
    int32_t u = 0, nlt = 0;
    for (int32_t i0 = 0; i0 < cnt; i0 += WAVE) {
        const int32_t i = i0 + ln;
        const int32_t x = i < cnt ? lds.cand[i] : 0;
        u += __popcll(ballot(i < cnt && x <= pos + SV_MIN_LENGTH / 2));
        nlt += __popcll(ballot(i < cnt && x < pos - SV_MIN_LENGTH / 2));
    }
    Band bd;
    bd.on = true;
    bd.f32 = true;                                          // every value >= 0
    bd.u = u + (below ? 1 : 0);
    bd.n_lt = nlt + (below ? 1 : 0);
    bd.n_le = below ? 1 : 0;
    bd.n_ge = above ? 1 : 0;
    bd.lo = W.lo;
    bd.hi = W.hi;
    int32_t sup = 0;
    return sort_and_vote<V_CONSENSUS>(lds.cand, lds.pre, cnt, pos, k, sup, &bd);
}

// The wave-wide window of any kind through the buckets when it qualifies: true and *r set; false:
// the caller takes the span-list path (refine_window).
template <bool COUNT>
__device__ __forceinline__ bool refine_any_bk(const KArgs &a, WinLds &lds, int kind, int chrom, uint32_t s, uint32_t e,
                                              uint32_t imp, unsigned long long *wk, uint32_t &r) {
    BkWin W;
    const int el = bk_eligible(a, kind, chrom, s, e, imp, W);
    if (el < 0) { r = SVT_NA; return true; }
    if (el == 0) return false;
    int32_t v;
    if (kind == K_INS) v = refine_window_bk<K_INS, COUNT>(a, lds, chrom - 1, W, imp, wk);
    else if (kind == K_START) v = refine_window_bk<K_START, COUNT>(a, lds, chrom - 1, W, imp, wk);
    else v = refine_window_bk<K_END, COUNT>(a, lds, chrom - 1, W, imp, wk);
    if (v == BK_FALLBACK) return false;
    r = (uint32_t)v;
    return true;
}

// ---- the build side's shared filing (svt_bucket_build.inc, and svt_index.inc's stream walk when a
// range's staged events overflowed: it files them straight from the walk)
// The tables are [array][nbk + 1] (array A's bucket g at A * (nbk + 1) + g), the events of all four
// arrays one buffer (the extents index it): an array is integer arithmetic, not a pointer select.
struct BkBuild {
    uint4 *ev;
    const uint32_t *off;          // the extents (filing pass)
    uint32_t *cur;                // filing: the cursors; counting: the counts (the zeroed extents' buffer)
    int32_t *pmx;                 // counting: per bucket the maximum BELOW key (-1: none)
    uint32_t *maxd;               // counting: per contig the longest D > 50 op
    const uint64_t *cbase;
    const uint32_t *cnb;
    uint64_t nbk;
    uint32_t k;                   // filing: the build's epoch (cursors hold k * count)
    uint32_t n_ev;                // the events' buffer (a bound for the slots of a failed extent check)
    uint32_t *err;
};

template <bool COUNT>
__device__ __forceinline__ void bk_put(const BkBuild &b, int A, uint32_t tid, uint32_t v, const uint4 &e, int32_t key) {
    const uint32_t nb = b.cnb[tid];
    const uint64_t g = (uint64_t)A * (b.nbk + 1) + b.cbase[tid] + (uint64_t)min(v >> BKS, nb - 1u);
    if (COUNT) {
        atomicAdd(&b.cur[g], 1u);
        if (A < 3) atomicMax(&b.pmx[g], key);
        return;
    }
    const uint32_t o0 = b.off[g], n = b.off[g + 1] - o0;
    const uint32_t sl = atomicAdd(&b.cur[g], 1u) - b.k * n;
    if (sl >= n) {
        *b.err = 3u;
        return;
    }
    b.ev[o0 + sl] = e;
}

// One event of read (tid, pos) as the span lists hold it ({x, word, endpos, 0}, leading S {pos,
// SP_LEAD, endpos, walk end}): the read's pos goes into the free word, then the event is filed.
// BELOW keys (svt_bucket.inc): endpos; trailing S min(x, endpos); leading S its read's pos.
template <bool COUNT>
__device__ __forceinline__ void bk_event(const BkBuild &b, uint32_t tid, uint32_t pos, uint4 v) {
    const uint32_t op = v.y & 0xfu;
    if (op == SP_LEAD) {
        bk_put<COUNT>(b, BA_E, tid, v.w + 1u, v, (int32_t)v.x);        // refinement.c:210-220
        bk_put<COUNT>(b, BA_L, tid, v.x, v, 0);
        return;
    }
    v.w = pos;
    if (op == OP_INS) {
        bk_put<COUNT>(b, BA_I, tid, v.x, v, (int32_t)v.z);             // :299
    } else if (op == SP_TRAIL) {
        bk_put<COUNT>(b, BA_S, tid, v.x, v, (int32_t)min(v.x, v.z));   // :147-159
    } else {                                                           // D > 50: :124, :188
        bk_put<COUNT>(b, BA_S, tid, v.x, v, (int32_t)v.z);
        bk_put<COUNT>(b, BA_E, tid, v.x + (v.y >> 4) + 1u, v, (int32_t)v.z);
        if (COUNT) atomicMax(&b.maxd[tid], v.y >> 4);
    }
}

