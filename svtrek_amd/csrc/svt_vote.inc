// svt_vote.inc -- sort + vote, wave-wide (included by svt_engine.hip after svt_gather.inc): the LDS
// and register sorts, the exact band filter, consensus_pos and sliding_window_ins's vote, and
// vote_window with its spill path.

// ------------------------------------------------------------------ sort + vote (A8-A10)
// Bitonic sort of buf[0..N) (N power of two, padded with INT32_MAX) by one wave.
__device__ __forceinline__ void wave_bitonic_sort(int32_t *buf, int N) {
    const int ln = lane_id();
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = ln; i < N; i += WAVE) {
                int p = i ^ j;
                if (p > i) {
                    int32_t a = buf[i], b = buf[p];
                    bool up = (i & k) == 0;
                    if ((a > b) == up) { buf[i] = b; buf[p] = a; }
                }
            }
            wave_sync();
        }
    }
}

// Bitonic sort of buf[0..n), n <= 64*E, in registers: element i = k*64 + lane lives in x[k];
// exchanges at distance >= 64 stay inside a lane, shorter ones are lane-xor shuffles.
// Padding is INT32_MAX; one load and one store per element.
// NB < 64 (E == 1, n <= NB): the merge stages stop at block size NB; the padding above NB
// stays in place (every exchange of a stage with block size kk stays inside its block).
template <int E, int NB = E * WAVE>
__device__ __forceinline__ int32_t reg_bitonic_sort(int32_t *buf, int32_t n) {   // returns element ln
    const int ln = lane_id();
    int32_t x[E];
#pragma unroll
    for (int k = 0; k < E; k++) x[k] = k * WAVE + ln < n ? buf[k * WAVE + ln] : INT32_MAX;
#pragma unroll
    for (int kk = 2; kk <= NB; kk <<= 1) {
#pragma unroll
        for (int j = kk >> 1; j > 0; j >>= 1) {
            if (j >= WAVE) {
                const int kj = j / WAVE;
#pragma unroll
                for (int k = 0; k < E; k++) {
                    if (k & kj) continue;
                    const bool asc = ((k * WAVE + ln) & kk) == 0;
                    const int32_t a = x[k], b = x[k | kj];
                    x[k] = asc ? min(a, b) : max(a, b);
                    x[k | kj] = asc ? max(a, b) : min(a, b);
                }
            } else {
#pragma unroll
                for (int k = 0; k < E; k++) {
                    const int i = k * WAVE + ln;
                    const int32_t y = lane_xor(x[k], j);
                    x[k] = (((i & j) == 0) == ((i & kk) == 0)) ? min(x[k], y) : max(x[k], y);
                }
            }
        }
    }
    wave_sync();
#pragma unroll
    for (int k = 0; k < E; k++) buf[k * WAVE + ln] = x[k];
    return x[0];
}

__device__ __forceinline__ int32_t ref_abs(int32_t a) { return a < 0 ? -a : a; }   // refinement.h:41

__device__ __forceinline__ int32_t first_greater(const int32_t *buf, int32_t l, int32_t h, int64_t key) {
    while (l < h) {
        int32_t m = (l + h) >> 1;
        if ((int64_t)buf[m] > key) h = m; else l = m + 1;
    }
    return l;
}
__device__ __forceinline__ int32_t first_geq(const int32_t *buf, int32_t l, int32_t h, int64_t key) {
    while (l < h) {
        int32_t m = (l + h) >> 1;
        if ((int64_t)buf[m] >= key) h = m; else l = m + 1;
    }
    return l;
}

__device__ SVT_COLD int32_t mean_round(int64_t tot, int32_t cnt) {   // cold: the 64-bit division
    // (int)((uint64 total + count/2) / count), refinement.c:66
    uint64_t t = (uint64_t)tot + (uint64_t)(int64_t)(cnt / 2);
    return (int32_t)(uint32_t)(t / (uint64_t)(int64_t)cnt);
}

// mean_round of a cluster whose smallest value is `base`.  With base >= 0 every value is
// >= 0, the reference's uint64 total is the exact sum, and (sum + cnt/2) / cnt =
// base + (sum - cnt*base + cnt/2) / cnt: a 32-bit division whenever the offsets' sum fits.
__device__ __forceinline__ int32_t mean_cluster(int64_t tot, int32_t cnt, int32_t base) {
    if (base >= 0) {
        const int64_t d = tot - (int64_t)cnt * (int64_t)base;
        if (d < (int64_t)0x7fffffff) {
            const uint32_t q = ((uint32_t)d + (uint32_t)(cnt / 2)) / (uint32_t)cnt;
            return (int32_t)((uint32_t)base + q);
        }
    }
    return mean_round(tot, cnt);
}

// Band filter (exact): consensus_pos only ever reads elements within `range` of pos and
// their clusters (within ci of them), i.e. values in (pos - range - ci, pos + range + ci),
// plus three facts about the whole multiset: whether any element is <= pos+25 (where the
// left pass starts, lower_bound), its minimum (upper_bound's A[0] < pos-25 test and the
// right pass's first element) and its maximum (the right pass's start when that test
// fails).  Both passes stop at the first out-of-range element, and every element between
// the band and the pass start is out of range, so voting over the band's sorted elements
// with those three facts visits the same elements with the same clusters.  Requires
// range > 25 (the left start pos+25 is then inside the band) and |pos|, |values| < 2^30
// (the reference's int32 differences cannot wrap); otherwise the full multiset is voted.
struct Band {
    bool on = false;    // the vote runs over the band's elements (else over the full multiset)
    bool f32 = false;   // ... and every band element is >= 0: 32-bit cluster sums (vote<true>)
    int32_t u = 0;      // #elements <= pos+25 of the full multiset (the left pass start)
    int32_t n_lt = 0;   // #elements <  pos-25 (upper_bound's A[0] < pos-25 test)
    int32_t n_le = 0;   // #elements <= lo (is the full minimum inside the band?)
    int32_t n_ge = 0;   // #elements >= hi (is the full maximum inside the band?)
    int32_t lo = 0, hi = 0;   // the band: open interval (lo, hi)
};

// Compacts buf[0..n) (n <= 4*WAVE) to its band elements in place; returns their count.
// Counts only (ballots), no reductions; int32 compares throughout, since the band is only
// used when |pos| < 2^30 and range + max(ci, 0) <= 2^22 (so lo, hi fit) and every element
// is within +-2^30.
__device__ __forceinline__ int32_t band_filter(int32_t *buf, int32_t n, int32_t pos, const KParams &k, Band &bd) {
    constexpr int32_t LIM = 1 << 30, WMAX = 1 << 22;
    if (k.range <= SV_MIN_LENGTH / 2 || pos <= -LIM || pos >= LIM || k.range > WMAX || k.ci > WMAX - k.range ||
        k.ci < -WMAX)
        return n;
    const int ln = lane_id();
    const int32_t w = k.range + max(k.ci, 0);
    const int32_t lo = pos - w, hi = pos + w;
    constexpr int E = 4;
    int32_t x[E];
    int32_t u = 0, nlt = 0, nle = 0, nge = 0;
    uint64_t bad = 0, neg = 0;
#pragma unroll
    for (int q = 0; q < E; q++) {
        x[q] = 0;
        if (q * WAVE >= n) break;   // wave-uniform: blocks past n hold nothing
        const int i = q * WAVE + ln;
        const bool v = i < n;
        x[q] = v ? buf[i] : 0;
        u += __popcll(ballot(v && x[q] <= pos + SV_MIN_LENGTH / 2));
        nlt += __popcll(ballot(v && x[q] < pos - SV_MIN_LENGTH / 2));
        nle += __popcll(ballot(v && x[q] <= lo));
        nge += __popcll(ballot(v && x[q] >= hi));
        bad |= ballot(v && (x[q] <= -LIM || x[q] >= LIM));
        neg |= ballot(v && lo < x[q] && x[q] < hi && x[q] < 0);
    }
    if (bad) return n;
    bd.on = true;
    bd.f32 = neg == 0;
    bd.u = u; bd.n_lt = nlt; bd.n_le = nle; bd.n_ge = nge;
    bd.lo = lo; bd.hi = hi;
    wave_sync();
    int32_t cnt = 0;
#pragma unroll
    for (int q = 0; q < E; q++) {
        if (q * WAVE >= n) break;
        const int i = q * WAVE + ln;
        const bool keep = i < n && lo < x[q] && x[q] < hi;
        const uint64_t m = ballot(keep);
        if (keep) buf[cnt + (int32_t)mbcnt(m)] = x[q];
        cnt += (int32_t)__popcll(m);
    }
    wave_sync();
    return cnt;
}

// band_filter for any n (the spill slab, > 4*WAVE candidates): the same counts and the same
// in-place compaction, 64 elements per step (writes never pass the block being read).
__device__ __forceinline__ int32_t band_filter_large(int32_t *buf, int32_t n, int32_t pos, const KParams &k,
                                                     Band &bd) {
    constexpr int32_t LIM = 1 << 30, WMAX = 1 << 22;
    if (k.range <= SV_MIN_LENGTH / 2 || pos <= -LIM || pos >= LIM || k.range > WMAX || k.ci > WMAX - k.range ||
        k.ci < -WMAX)
        return n;
    const int ln = lane_id();
    const int32_t w = k.range + max(k.ci, 0);
    const int32_t lo = pos - w, hi = pos + w;
    int32_t u = 0, nlt = 0, nle = 0, nge = 0;
    uint64_t bad = 0, neg = 0;
    for (int32_t b = 0; b < n; b += WAVE) {
        const int32_t i = b + ln;
        const bool v = i < n;
        const int32_t x = v ? buf[i] : 0;
        u += __popcll(ballot(v && x <= pos + SV_MIN_LENGTH / 2));
        nlt += __popcll(ballot(v && x < pos - SV_MIN_LENGTH / 2));
        nle += __popcll(ballot(v && x <= lo));
        nge += __popcll(ballot(v && x >= hi));
        bad |= ballot(v && (x <= -LIM || x >= LIM));
        neg |= ballot(v && lo < x && x < hi && x < 0);
    }
    if (bad) return n;
    bd.on = true;
    bd.f32 = neg == 0;
    bd.u = u; bd.n_lt = nlt; bd.n_le = nle; bd.n_ge = nge;
    bd.lo = lo; bd.hi = hi;
    wave_sync();
    int32_t cnt = 0;
    for (int32_t b = 0; b < n; b += WAVE) {
        const int32_t i = b + ln;
        const int32_t x = i < n ? buf[i] : 0;
        const bool keep = i < n && lo < x && x < hi;
        const uint64_t m = ballot(keep);
        wave_sync();
        if (keep) buf[cnt + (int32_t)mbcnt(m)] = x;
        cnt += (int32_t)__popcll(m);
        wave_sync();
    }
    return cnt;
}

__device__ __forceinline__ int32_t first_greater32(const int32_t *buf, int32_t l, int32_t h, int32_t key) {
    while (l < h) {
        int32_t m = (l + h) >> 1;
        if (buf[m] > key) h = m; else l = m + 1;
    }
    return l;
}
__device__ __forceinline__ int32_t first_geq32(const int32_t *buf, int32_t l, int32_t h, int32_t key) {
    while (l < h) {
        int32_t m = (l + h) >> 1;
        if (buf[m] >= key) h = m; else l = m + 1;
    }
    return l;
}

// consensus_pos (refinement.c:41-101) on sorted A[0..n) with prefix sums P[0..n].
// reg: x0 holds A[lane] for lanes < min(n, 64) (the register sorts), read instead of LDS.
// F32: A is a band with every element >= 0 and P holds 32-bit sums of A[j] - A0 (A0 = A[0]):
// the reference's rounded uint64 mean (sum + c/2) / c of a cluster of non-negative values is
// then A0 + (its offset sum + c/2) / c exactly, in 32 bits (offset sums < 2^31, band_filter).
template <bool F32>
__device__ __forceinline__ int32_t vote(const int32_t *A, const void *Pv, int32_t n, int32_t pos, const KParams &k,
                                        int32_t x0, bool reg, const Band &bd, int32_t A0) {
    const int64_t *P = reinterpret_cast<const int64_t *>(Pv);
    const uint32_t *P32 = reinterpret_cast<const uint32_t *>(Pv);
    const int ln = lane_id();
    const int32_t ci = k.ci, range = k.range;
    int32_t valL = -1, maxL = k.min_count - 1, distL = 0x7fffffff;
    int32_t valR = -1, maxR = k.min_count - 1, distR = 0x7fffffff;

    // lower_bound(A, n, pos+25): (#elements <= pos+25) - 1, clamped at 0  (refinement.c:3-10)
    int32_t u = 0;
    for (int32_t b = 0; b < n; b += WAVE) {
        int32_t i = b + ln;
        u += __popcll(ballot(i < n && (reg && b == 0 ? x0 : A[i]) <= pos + SV_MIN_LENGTH / 2));
    }
    int32_t p = u == 0 ? 0 : u - 1;
    if (bd.on) {   // A = the band of the full multiset (see Band): start where the full pass would
        p = bd.u == 0 ? 0 : u == 0 ? -1 : u - 1;   // u >= 1 elements <= pos+25 but none in the band:
        if (n == 0) p = -1;                         // the full pass stops at once (below the band)
    }

    // left pass: i = p, p-1, ... while |pos - A[i]| < range   (refinement.c:58-77)
    for (int32_t top = p; top >= 0; top -= WAVE) {
        int32_t i = top - ln;
        bool inr = i >= 0 && ref_abs(pos - A[i < 0 ? 0 : i]) < range;
        uint64_t stop = ballot(!inr);
        int lim = stop ? __builtin_ctzll(stop) : WAVE;   // lanes [0, lim) are in the pass
        int32_t cnt = 0, cand = 0;
        if (ln < lim) {
            int32_t a = A[i];
            if (F32) {
                const int32_t kk = first_geq32(A, 0, i, a - ci);   // contiguous j<i with a <= A[j]+ci
                cnt = i - kk + 1;
                cand = A0 + (int32_t)((P32[i + 1] - P32[kk] + (uint32_t)(cnt / 2)) / (uint32_t)cnt);
            } else {
                int32_t kk = first_geq(A, 0, i, (int64_t)a - ci);   // contiguous j<i with a <= A[j]+ci
                cnt = i - kk + 1;
                cand = mean_cluster(P[i + 1] - P[kk], cnt, A[kk]);
            }
        }
        // the greedy accept in pass order, visiting only elements whose count beats maxL
        const int32_t dd = ref_abs(pos - cand);
        for (int l = -1;;) {
            const uint64_t cm = ballot(ln < lim && ln > l && cnt > maxL);
            if (!cm) break;
            l = __builtin_ctzll(cm);
            const int32_t c = rdlane_i(cnt, l), v = rdlane_i(cand, l), d = rdlane_i(dd, l);
            if (d < ci) return v;                        // early return, refinement.c:67-68
            if (d < distL) { maxL = c; valL = v; distL = d; }
        }
        if (stop) break;
    }

    // upper_bound(A, n, pos-25): 0 if A[0] < pos-25 else n-1   (refinement.c:12-19)
    int32_t q = (n > 0 && (reg ? rdlane_i(x0, 0) : A[0]) < pos - SV_MIN_LENGTH / 2) ? 0 : n - 1;
    if (bd.on)   // the full multiset's A[0] / A[n-1]: in the band they are A's first / last element
        q = bd.n_lt > 0 ? (bd.n_le == 0 ? 0 : n) : (bd.n_ge == 0 ? n - 1 : n);
    for (int32_t bot = q; bot < n; bot += WAVE) {
        int32_t i = bot + ln;
        const int32_t ai = reg && bot == 0 ? x0 : A[i < n ? i : 0];
        bool inr = i < n && ref_abs(pos - ai) < range;
        uint64_t stop = ballot(!inr);
        int lim = stop ? __builtin_ctzll(stop) : WAVE;
        int32_t cnt = 0, cand = 0;
        if (ln < lim) {
            int32_t a = ai;
            if (F32) {
                const int32_t m = first_greater32(A, i + 1, n, a + ci);   // contiguous j>i with A[j] <= a+ci
                cnt = m - i;
                cand = A0 + (int32_t)((P32[m] - P32[i] + (uint32_t)(cnt / 2)) / (uint32_t)cnt);
            } else {
                int32_t m = first_greater(A, i + 1, n, (int64_t)a + ci);   // contiguous j>i with A[j] <= a+ci
                cnt = m - i;
                cand = mean_cluster(P[m] - P[i], cnt, a);
            }
        }
        const int32_t dd = ref_abs(pos - cand);
        for (int l = -1;;) {
            const uint64_t cm = ballot(ln < lim && ln > l && cnt > maxR);
            if (!cm) break;
            l = __builtin_ctzll(cm);
            const int32_t c = rdlane_i(cnt, l), v = rdlane_i(cand, l), d = rdlane_i(dd, l);
            if (d < ci) return v;                        // refinement.c:88-89
            if (d < distR) { maxR = c; valR = v; distR = d; }
        }
        if (stop) break;
    }
    return distL < distR ? valL : valR;   // refinement.c:100
}

// sliding_window_ins's vote (sliding_window.c:65-84) on sorted A[0..n) with prefix sums
// P[0..n]: for i = 0, slide, 2*slide, ...: support = #{j >= i : A[j] - A[i] <= ws}; the
// first i reaching the largest support >= min_count wins, its candidate is the rounded
// mean of A[i..i+support) in the reference's 32-bit int arithmetic (sum wraps mod 2^32).
__device__ __forceinline__ int32_t sw_vote(const int32_t *A, const int64_t *P, int32_t n, const KParams &k,
                                           int32_t &support_out) {
    const int ln = lane_id();
    const int32_t ws = k.sw_window, slide = k.sw_slide;
    const int32_t nstart = (n + slide - 1) / slide;
    int32_t best_sup = 0, best_i = -1;
    for (int32_t b = 0; b < nstart; b += WAVE) {
        const int32_t t = b + ln;
        int32_t sup = 0, i = 0;
        if (t < nstart) {
            i = t * slide;
            sup = first_greater(A, i, n, (int64_t)A[i] + ws) - i;         // :71-75
        }
        const bool ok = sup >= k.min_count;                                  // :76
        // wave max of qualifying supports; ties -> the smallest i (strict > in :76)
        int32_t m = wave_scan_max(ok ? sup : -1);
        m = rdlane_i(m, WAVE - 1);
        if (m > best_sup) {
            const uint64_t at = ballot(ok && sup == m);
            best_sup = m;
            best_i = rdlane_i(i, __builtin_ctzll(at));
        }
    }
    support_out = best_sup;
    if (best_i < 0) return -1;
    const uint32_t sum = (uint32_t)(uint64_t)(P[best_i + best_sup] - P[best_i]);      // :78-81, int wrap
    return (int32_t)(sum + (uint32_t)(best_sup / 2)) / best_sup;                      // :82
}

constexpr int V_CONSENSUS = 0, V_SLIDING = 1;

// Sort + prefix sums + vote over buf[0..n) with scratch for P (n+1 int64).
// LARGE: n > 4*WAVE is known (the spill slab): only the global bitonic + the int64 vote.
template <int VOTE, bool LARGE = false>
__device__ __forceinline__ int32_t sort_and_vote(int32_t *buf, int64_t *P, int32_t n, int32_t pos, const KParams &k,
                                                 int32_t &support, const Band *given = nullptr) {
    const int ln = lane_id();
    Band bd;
    if (given) bd = *given;   // buf already holds the band (band_filter_large)
    else if (!LARGE && VOTE == V_CONSENSUS && n <= 4 * WAVE) n = band_filter(buf, n, pos, k, bd);
    int32_t x0 = 0;   // sorted element ln, from the register sorts (no LDS read-back below)
    if (LARGE) {
        int N = 1;
        while (N < n) N <<= 1;
        for (int i = n + ln; i < N; i += WAVE) buf[i] = INT32_MAX;
        wave_sync();
        wave_bitonic_sort(buf, N);
    } else if (n <= 16) x0 = reg_bitonic_sort<1, 16>(buf, n);
    else if (n <= 32) x0 = reg_bitonic_sort<1, 32>(buf, n);
    else if (n <= WAVE) x0 = reg_bitonic_sort<1>(buf, n);
    else if (n <= 2 * WAVE) x0 = reg_bitonic_sort<2>(buf, n);
    else if (n <= 4 * WAVE) x0 = reg_bitonic_sort<4>(buf, n);
    else {
        int N = 1;
        while (N < n) N <<= 1;
        for (int i = n + ln; i < N; i += WAVE) buf[i] = INT32_MAX;
        wave_sync();
        wave_bitonic_sort(buf, N);
    }
    if (!LARGE && VOTE == V_CONSENSUS && bd.on && bd.f32) {   // 32-bit offset sums (see vote<true>)
        uint32_t *P32 = reinterpret_cast<uint32_t *>(P);
        const int32_t A0 = n > 0 ? rdlane_i(x0, 0) : 0;
        uint32_t carry = 0;
        if (ln == 0) P32[0] = 0;
        for (int32_t b = 0; b < n; b += WAVE) {
            const int32_t i = b + ln;
            const uint32_t x = i < n ? (uint32_t)((b == 0 ? x0 : buf[i]) - A0) : 0u;
            const uint32_t sc = carry + wave_scan_add(x);
            if (i < n) P32[i + 1] = sc;
            carry = rdlane(sc, WAVE - 1);
        }
        wave_sync();
        return vote<true>(buf, P32, n, pos, k, x0, true, bd, A0);
    }
    int64_t carry = 0;
    if (ln == 0) P[0] = 0;
    for (int32_t b = 0; b < n; b += WAVE) {
        int32_t i = b + ln;
        int64_t x = i < n ? (int64_t)(!LARGE && b == 0 && n <= 4 * WAVE ? x0 : buf[i]) : 0;
        int64_t s = carry + wave_scan_add64(x);
        if (i < n) P[i + 1] = s;
        carry = (int64_t)rdlane64((uint64_t)s, WAVE - 1);
    }
    wave_sync();
    if (VOTE == V_SLIDING) return sw_vote(buf, P, n, k, support);
    return vote<false>(buf, P, n, pos, k, x0, !LARGE && n <= 4 * WAVE, bd, 0);
}

struct WinLds {
    int64_t pre[CAP + 1];         // the wave-wide vote's prefix sums
    int32_t cand[CAP];
    int32_t ncand;
};

// After the gather: n candidates in lds.cand (the first CAP of them) -> consensus_pos.
template <int KIND, bool COUNT, int VOTE>
__device__ __forceinline__ int32_t vote_window(const KArgs &a, WinLds &lds, int chrom, uint32_t s, uint32_t e,
                                               uint32_t imprecise, int32_t n, unsigned long long *wk, int32_t &support) {
    support = 0;
    if (n < a.prm.min_count) return -1;                    // refinement.c:43-45 (sliding: no support >= min_count)
    if (n <= CAP) return sort_and_vote<VOTE>(lds.cand, lds.pre, n, (int32_t)imprecise, a.prm, support);
    // spill: a slab for N ints + (n+1) int64 from the device pool, then re-gather into it
    if (COUNT && lane_id() == 0) wk[W_SPILLED] += 1;
    int N = 1;
    while (N < n) N <<= 1;
    unsigned long long words = (unsigned long long)N + 2ull * (unsigned long long)(n + 2);
    // the pool restarts for every launch: a head word tagged with another launch's epoch
    // counts as empty (no per-launch reset on the host)
    unsigned long long base = 0;
    if (lane_id() == 0) {
        unsigned long long old = __hip_atomic_load(a.pool_head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), seen;
        do {
            seen = old;
            base = (uint32_t)(seen >> 40) == a.epoch ? (seen & ((1ull << 40) - 1ull)) : 0ull;
            old = atomicCAS(a.pool_head, seen, ((unsigned long long)a.epoch << 40) | (base + words));
        } while (old != seen);
    }
    base = rdlane64(base, 0);
    if (base + words > a.pool_words) {
        if (lane_id() == 0) atomicOr(a.status, 1);
        return -1;
    }
    int32_t *g = a.pool + base;
    int64_t *gp = (int64_t *)(a.pool + ((base + (unsigned long long)N + 1ull) & ~1ull));
    WinStats st2;
    Sink s2{g, N, &lds.ncand};
    gather<KIND, false>(a, chrom - 1, s, e, s2, st2);
    if (VOTE == V_CONSENSUS) {   // the exact band first: usually small enough for the register sort
        Band bd;
        const int32_t nb = band_filter_large(g, n, (int32_t)imprecise, a.prm, bd);
        if (bd.on && nb <= CAP) {
            for (int32_t i = lane_id(); i < nb; i += WAVE) lds.cand[i] = g[i];
            wave_sync();
            return sort_and_vote<VOTE>(lds.cand, lds.pre, nb, (int32_t)imprecise, a.prm, support, &bd);
        }
        if (bd.on) return sort_and_vote<VOTE, true>(g, gp, nb, (int32_t)imprecise, a.prm, support, &bd);
    }
    return sort_and_vote<VOTE, true>(g, gp, n, (int32_t)imprecise, a.prm, support);
}
