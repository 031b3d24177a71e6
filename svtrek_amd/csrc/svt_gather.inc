// svt_gather.inc -- a window's candidates, wave-wide (included by svt_engine.hip after svt_wave.inc):
// the candidate sink, the region query (A3), the per-read replay of the reference's walk, and the
// span walk over the per-read event lists with its gather() front.

// ------------------------------------------------------------------ candidate sink
// Where a window's candidates go.  Their order is irrelevant (the multiset is sorted before
// the vote).  The span walk fills buf by ballot ranks and stores cnt once (span_walk); the
// per-read replay appends with an LDS atomic per candidate (push), under any divergence.
struct Sink {
    int32_t *buf;   // LDS or a global spill slab
    int32_t cap;
    int32_t *cnt;   // LDS counter: candidates seen (may exceed cap -> spill re-run)
    __device__ __forceinline__ void push1(int32_t val) {
        int idx = atomicAdd(cnt, 1);
        if (idx < cap) buf[idx] = val;
    }
    __device__ __forceinline__ void push(bool pred, int32_t val) {
        if (pred) push1(val);
    }
};

struct WinStats {
    unsigned long long reads = 0, ops = 0;
    // span walk's own reads (svt_count_work): see svt_work
    unsigned long long queries = 0, probe = 0, range = 0, lreads = 0, lentries = 0, stops = 0, stopch = 0;
    unsigned long long squeries = 0, span = 0;   // span walk (COUNT builds)
};

template <int KIND>
__device__ __forceinline__ bool is_candidate_op(uint32_t op, uint32_t len) {
    if (KIND == K_INS) return op == OP_INS && (uint32_t)SV_MIN_LENGTH <= len;   // refinement.c:299
    return op == OP_DEL && (uint32_t)SV_MIN_LENGTH < len;                       // refinement.c:124,:188
}

// Per-read walk, 64 ops per step, replaying the reference's uint32 position arithmetic
// exactly (refinement.c:118-159 / :184-221 / :295-318).  Used for reads whose walk could
// wrap 2^32 (never in practice: gather_perread) and by the COUNT builds.
// SinkT: the LDS candidate sink, or svt_evidence.inc's counting sink (push(pred, val) per lane).
template <int KIND, bool COUNT, typename SinkT>
__device__ __forceinline__ void walk_read(const uint32_t *__restrict__ cigar, uint64_t off, uint32_t n, uint32_t rpos,
                          uint32_t clip, uint32_t s, uint32_t e, SinkT &sink, WinStats &st) {
    const int ln = lane_id();
    uint32_t carry = rpos;
    bool broke = false;
    uint32_t stop_rp = 0;
    uint32_t walked = n;
    for (uint32_t cb = 0; cb < n; cb += WAVE) {
        uint32_t i = cb + (uint32_t)ln;
        bool v = i < n;
        uint32_t w = v ? cigar[off + i] : 0u;
        uint32_t op = w & 0xfu, len = w >> 4;
        uint32_t adv = (op != OP_INS && op != OP_SOFT) ? len : 0u;   // refinement.c:141
        uint32_t after = carry + wave_scan_add(adv);
        uint32_t before = after - adv;
        uint64_t bm = ballot(v && after > e);                         // refinement.c:145
        int fb = bm ? __builtin_ctzll(bm) : WAVE;
        bool hit = v && ln <= fb && is_candidate_op<KIND>(op, len);
        sink.push(hit, KIND == K_END ? (int32_t)(before + len + 1u) : (int32_t)before);   // :198 / :134
        if (bm) {
            broke = true;
            stop_rp = rdlane(after, fb);
            walked = cb + (uint32_t)fb + 1u;
            break;
        }
        carry = rdlane(after, WAVE - 1);
    }
    if (KIND == K_START) {   // trailing soft clip, refinement.c:120,:147-159
        bool c = (clip & SVT_CLIP_LAST_S) && !broke && s <= carry && carry <= e;
        sink.push(c && ln == 0, (int32_t)carry);
    } else if (KIND == K_END) {   // leading soft clip, refinement.c:210-221 (rp = walked position)
        bool c = (clip & SVT_CLIP_FIRST_S) && (int64_t)s <= (int64_t)(int32_t)rpos &&
                 (int64_t)(int32_t)rpos <= (int64_t)e;
        sink.push(c && ln == 0, (int32_t)((broke ? stop_rp : carry) + 1u));
    }
    if (COUNT) {
        st.reads++;
        uint64_t wk = walked;
        if (KIND == K_START && (n == 0 || (broke && walked < n))) wk++;   // cigar[n-1] test
        if (KIND == K_END && n == 0) wk++;                                 // cigar[0] test
        st.ops += wk;
    }
}

// ------------------------------------------------------------------ read range (A3)
// sam_itr_queryi(idx, chrom-1, inter.start-1, inter.end-1) (refinement.c:114): the reads
// [lo, hi) of contig tid may overlap [beg, end) (each still needs endpos > beg), with
//   hi = first read with pos >= end,  lo = first read with emax > beg  (emax = prefix max
//   of endpos, so every read before lo ends at or before beg).
// The bucket table gives, per 4 kb bucket b, {first read with pos >= b*4096, first read with
// emax >= b*4096}; each bound then lies inside one bucket, and the two searches share two
// dependent steps: 4 bucket words, then one 64-lane probe each of pos[] and emax[].
__device__ __forceinline__ int64_t probe_first(int64_t l, int64_t h, bool hit_in_lane, bool lane_valid) {
    const uint64_t m = ballot(lane_valid && hit_in_lane);
    return m ? l + __builtin_ctzll(m) : h;
}

__device__ __forceinline__ bool read_range(const DevPileup &P, int tid, int64_t beg, int64_t end, int64_t &lo,
                                           int64_t &hi, WinStats *st = nullptr) {
    if (tid < 0 || tid >= P.n_targets || end <= beg) return false;   // no reads (A3)
    const int64_t ra = P.tid_off[tid], nr = P.tid_off[tid + 1] - ra;
    if (nr == 0) return false;
    const int64_t b0 = P.bkt_off[tid], nb = P.bkt_off[tid + 1] - b0;   // last bucket = {nr, nr}
    const int ln = lane_id();
    const int64_t bi = min((ln < 2 ? end >> BKT_SHIFT : beg >> BKT_SHIFT) + (ln & 1), nb - 1);
    const uint2 bw = ln < 4 ? P.bkt[b0 + bi] : make_uint2(0, 0);
    const int64_t hl = rdlane(bw.x, 0), hh = rdlane(bw.x, 1), ll = rdlane(bw.y, 2), lh = rdlane(bw.y, 3);
    const int32_t *pos = P.pos + ra, *emax = P.emax + ra;
    const bool vh = hl + ln < hh, vl = ll + ln < lh;
    const int32_t pv = vh ? pos[hl + ln] : 0, ev = vl ? emax[ll + ln] : 0;
    int64_t h = probe_first(hl, hh, (int64_t)pv >= end, vh);
    int64_t l = probe_first(ll, lh, (int64_t)ev > beg, vl);
    if (hh - hl > WAVE) h = wave_partition_point(hl, hh, [&](int64_t r) { return (int64_t)pos[r] >= end; });
    if (lh - ll > WAVE) l = wave_partition_point(ll, lh, [&](int64_t r) { return (int64_t)emax[r] > beg; });
    if (st) {   // COUNT builds: the bucket words + each search's entries up to its boundary
        st->queries++;
        st->probe += (unsigned long long)((h - hl) + (h < hh ? 1 : 0) + (l - ll) + (l < lh ? 1 : 0));
    }
    lo = ra + l;
    hi = ra + h;
    return lo < hi;
}

// ------------------------------------------------------------------ per-read gather
template <int KIND, bool COUNT, typename SinkT>
__device__ __forceinline__ void gather_perread(const DevPileup &P, int tid, uint32_t s, uint32_t e, SinkT &sink, WinStats &st) {
    const int64_t beg = (int64_t)(uint32_t)(s - 1u), end = (int64_t)(uint32_t)(e - 1u);
    int64_t lo, hi;
    if (!read_range(P, tid, beg, end, lo, hi)) return;
    const int ln = lane_id();
    for (int64_t base = lo; base < hi; base += WAVE) {
        int64_t r = base + ln;
        bool valid = r < hi;
        uint4 rc = valid ? P.rec[r] : make_uint4(0, 0, 0, 0);
        bool ov = valid && (int64_t)(int32_t)rc.y > beg;   // pos < end holds below hi (hts_itr_next)
        uint64_t m = ballot(ov);
        while (m) {
            int l = __builtin_ctzll(m);
            m &= m - 1;
            uint32_t z = rdlane(rc.z, l);
            walk_read<KIND, COUNT>(P.cigar, P.off64[base + l], z & NCIG_MASK, rdlane(rc.x, l), z >> 30, s, e, sink,
                                   st);
        }
    }
}

// ------------------------------------------------------------------ span walk
// The reads [lo, hi) of a window own one contiguous span of the D (or I) event list, and
// every event carries what its tests need (its read's endpos for the overlap test of
// hts_itr_next), so a window is: region query, the span's two bounds, then ONE filter over
// the span, every load of a 256-event batch issued at once (no per-read dependent chain).
// An op is processed by the reference walk iff the walk position before it is <= inter.end
// (positions only grow along a read, refinement.c:145), so a candidate event counts iff
// x <= e; the soft-clip events follow refinement.c:147-159 (trailing S: no break, s <= walk
// end <= e) and :210-220 (leading S, s <= pos <= e: walk end + 1, or -- the walk passes e --
// the position after the break op + 1, which votes as e + 2: KParams::sent_ok).
constexpr int SPAN_U = 4;   // 16-B event loads in flight per lane

// The span walk's own reads, for svt_count_work: the region query and the events of the span.
template <int KIND>
__device__ __forceinline__ void span_count(const DevPileup &P, int tid, uint32_t s, uint32_t e, WinStats &st) {
    const int64_t beg = (int64_t)(uint32_t)(s - 1u), end = (int64_t)(uint32_t)(e - 1u);
    int64_t lo, hi;
    if (!read_range(P, tid, beg, end, lo, hi, &st)) return;
    const uint64_t *off = KIND == K_INS ? P.spoffI : P.spoffD;
    st.squeries++;
    st.span += off[hi] - off[lo];
}

// read_range (A3) with the span bounds read in the same dependent step as the pos/emax
// probes: each probe lane also loads the span offset of its read, and the bounds are taken
// from the lanes where the two searches end (one HBM round trip less per window).  Wider
// bucket ranges fall back to read_range + one more step.
template <int KIND>
__device__ __forceinline__ bool span_query(const DevPileup &P, int tid, int64_t beg, int64_t end, uint64_t &E0,
                                           uint64_t &E1) {
    if (tid < 0 || tid >= P.n_targets || end <= beg) return false;   // no reads (A3)
    const int64_t ra = P.tid_off[tid], nr = P.tid_off[tid + 1] - ra;
    if (nr == 0) return false;
    const uint64_t *off = KIND == K_INS ? P.spoffI : P.spoffD;
    const int64_t b0 = P.bkt_off[tid], nb = P.bkt_off[tid + 1] - b0;   // last bucket = {nr, nr}
    const int ln = lane_id();
    const int64_t bi = min((ln < 2 ? end >> BKT_SHIFT : beg >> BKT_SHIFT) + (ln & 1), nb - 1);
    const uint2 bw = ln < 4 ? P.bkt[b0 + bi] : make_uint2(0, 0);
    const int64_t hl = rdlane(bw.x, 0), hh = rdlane(bw.x, 1), ll = rdlane(bw.y, 2), lh = rdlane(bw.y, 3);
    if (hh - hl >= WAVE || lh - ll >= WAVE) {   // wide bucket: the general search, then the bounds
        int64_t lo, hi;
        if (!read_range(P, tid, beg, end, lo, hi)) return false;
        const uint64_t ob = ln < 2 ? off[ln ? hi : lo] : 0ull;
        E0 = rdlane64(ob, 0);
        E1 = rdlane64(ob, 1);
        return true;
    }
    // lanes [0, hh-hl] cover the hi candidates hl .. hh, lanes [0, lh-ll] the lo candidates
    const bool vh = hl + ln <= hh, vl = ll + ln <= lh;
    const int64_t rh = ra + (vh ? hl + ln : hl), rl = ra + (vl ? ll + ln : ll);
    const int32_t pv = vh && hl + ln < hh ? P.pos[rh] : 0, ev = vl && ll + ln < lh ? P.emax[rl] : 0;
    const uint64_t oh = off[rh], ol = off[rl];
    const uint64_t mh = ballot(vh && hl + ln < hh && (int64_t)pv >= end);
    const uint64_t ml = ballot(vl && ll + ln < lh && (int64_t)ev > beg);
    const int kh = mh ? __builtin_ctzll(mh) : (int)(hh - hl), kl = ml ? __builtin_ctzll(ml) : (int)(lh - ll);
    if (ll + kl >= hl + kh) return false;
    E1 = rdlane64(oh, kh);
    E0 = rdlane64(ol, kl);
    return true;
}

// One span event's test for window [s, e] (query beg = s-1): it is a candidate with value val.
// A leading-S read whose walk passes e (refine_end's stop, :210-221) is one at e + 2.
template <int KIND>
__device__ __forceinline__ bool span_cand(const uint4 &v, uint32_t s, uint32_t e, int32_t beg32, uint32_t &val) {
    const uint32_t x = v.x, op = v.y & 0xfu, len = v.y >> 4;
    const bool ovl = (int32_t)v.z > beg32;   // hts_itr_next overlap; pos < end holds below hi
    val = x;
    if (KIND == K_INS) return ovl && op == OP_INS && x <= e;                   // refinement.c:299
    if (KIND == K_START) return ovl && x <= e && (op == OP_DEL || (op == SP_TRAIL && s <= x));   // :124 / :147-159
    const bool lead = op == SP_LEAD && ovl && s <= x && x <= e;                // :210-220
    val = op == OP_DEL ? x + len + 1u : v.w > e ? e + 2u : v.w + 1u;
    return (ovl && x <= e && op == OP_DEL) || lead;                            // :188-199
}

template <int KIND>
__device__ __forceinline__ void span_walk(const DevPileup &P, uint32_t s, uint32_t e, uint64_t E0, uint64_t E1,
                                          Sink &sink) {
    const int32_t beg32 = (int32_t)(uint32_t)(s - 1u);   // yielded reads: beg < end <= 2^30
    const int ln = lane_id();
    const uint4 *ev = KIND == K_INS ? P.spI : P.spD;
    int32_t cnt = 0;   // candidates appended so far (wave-uniform)
    for (uint64_t b = E0; b < E1; b += SPAN_U * WAVE) {
        uint4 v[SPAN_U];
        const uint64_t left = E1 - b;   // events from b on (wave-uniform): the u-slots past them are skipped
        // loads with clamped indices and no branches, so that all of them are in flight
        // before the first is used; lanes past E1 are masked below
#pragma unroll
        for (int u = 0; u < SPAN_U; u++) {
            const uint64_t j = b + (uint64_t)(u * WAVE + ln);
            if ((uint64_t)(u * WAVE) < left) v[u] = ev[j < E1 ? j : E1 - 1];
        }
#pragma unroll
        for (int u = 0; u < SPAN_U; u++) {
            if ((uint64_t)(u * WAVE) >= left) break;
            if ((uint64_t)(u * WAVE + ln) >= left) v[u] = make_uint4(0, 0, 0, 0);   // zero event: no candidate
            uint32_t val;
            const bool c = span_cand<KIND>(v[u], s, e, beg32, val);
            const uint64_t m = ballot(c);
            const int32_t idx = cnt + (int32_t)mbcnt(m);
            if (c && idx < sink.cap) sink.buf[idx] = (int32_t)val;
            cnt += (int32_t)__popcll(m);
        }
    }
    if (ln == 0) *sink.cnt = cnt;
}

// The wave-wide gather of one window: the span walk, or the reference's own per-read walk for
// windows ending at or past WEXACT and for refine_end windows whose leading-S stops cannot
// vote as e + 2 (!sent_ok).
template <int KIND, bool COUNT>
__device__ __forceinline__ void gather_span(const DevPileup &P, const KParams &k, int tid, uint32_t s, uint32_t e,
                                            Sink &sink, WinStats &st) {
    if (COUNT) {   // diagnostic: the reference's work by the exact per-read walk + what the span walk reads
        gather_perread<KIND, true>(P, tid, s, e, sink, st);
        if (e < WEXACT) span_count<KIND>(P, tid, s, e, st);
        return;
    }
    if (e >= WEXACT || (KIND == K_END && !k.sent_ok)) { gather_perread<KIND, COUNT>(P, tid, s, e, sink, st); return; }
    const int64_t beg = (int64_t)(uint32_t)(s - 1u), end = (int64_t)(uint32_t)(e - 1u);
    uint64_t E0, E1;
    if (!span_query<KIND>(P, tid, beg, end, E0, E1)) return;
    span_walk<KIND>(P, s, e, E0, E1, sink);
}

// The window gather: the span walk (gather_span) into a zeroed sink; returns the candidates seen.
template <int KIND, bool COUNT>
__device__ __forceinline__ int32_t gather(const KArgs &a, int tid, uint32_t s, uint32_t e, Sink &sink, WinStats &st) {
    if (lane_id() == 0) *sink.cnt = 0;
    wave_sync();
    gather_span<KIND, COUNT>(a.pile, a.prm, tid, s, e, sink, st);
    wave_sync();
    return uniform_i(*sink.cnt);
}
