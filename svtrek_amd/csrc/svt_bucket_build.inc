// svt_bucket_build.inc -- the value-bucketed event index, build side (included by svt_engine.hip
// after svt_index2.inc; the refine side and the why are in svt_bucket.inc).
//
// Every candidate event of the pileup -- the reference's per-read walk (refinement.c:118-159 /
// :184-221 / :295-318) done once per read -- is FILED by the value it votes with: a D > 50 op into
// S (by its walk position x) and E (by x + len + 1), a trailing-S marker into S, a leading-S marker
// into E (by walk end + 1) and L (by read start), an I >= 50 op into I.  Its slot within its bucket
// comes from an atomic cursor; the order inside a bucket is whatever the atomics give (a window
// tests every event of its buckets and the vote sorts the band: nothing depends on it).
//
// Two builds:
//   * the first, at svt_load_pileup: a counting pass (per bucket its events and the maximum of the
//     BELOW key, per contig its longest D > 50 op), the extents (an exclusive scan) and the prefix
//     maxima on the host, then a filing pass;
//   * every later one (svt_reindex, bench.py's step): the filing pass alone.  The extents depend on
//     the pileup only, like the span lists' sizes (and the BAI the reference's queries read): each
//     rebuild walks every read again and files every event again, and an event whose slot falls
//     outside its bucket's extent is an engine error (status word 2 = 3, svt_sync).
// Cursors without a reset: bucket g's cursor holds k * n_g before build k (n_g its events), so a
// slot is atomicAdd(cursor) - k * n_g (mod 2^32).  A build captured into a graph (replayed at any
// time) files through its own cursors instead, zeroed by bk_zero_kernel at the graph's head.
// Decompositions: short reads (the lane-per-read index, cfg4) are walked one lane per read straight
// from the CIGAR stream (ixb_lane_kernel) -- no census, no span lists; long reads: the stream walk's
// one pass stages each range's events and ixb_copy_kernel files the stage.

// Filing one event per lane, wave-wide, for a wave whose events all lie in one contig (bucket base
// cb, nbt buckets): the events of one locus come from neighbouring reads -- the same wave -- and go
// to the same few buckets, so the lanes of a bucket take their slots with ONE atomic (the lowest such
// lane adds their count; each lane's slot is the returned base + its rank among them) instead of
// each lane's own: same-address atomics serialise in the L2 (cfg4's filing pass 2.13 ms with one
// atomic per event).  Both filings of an event (D > 50: S and E; leading S: E and L) in turn.
#ifndef SVT_BK_AGG
#define SVT_BK_AGG 1   // 0 (A/B builds): one atomic per lane, no grouping -- 2.08 vs 1.28 ms on cfg4 (profiles/r06_G)
#endif
template <bool COUNT>
__device__ __forceinline__ void bk_file_wave(const BkBuild &b, uint64_t cb, uint32_t nbt, const uint4 &v, bool valid) {
    const int ln = lane_id();
    const uint32_t op = v.y & 0xfu;
#pragma unroll
    for (int f = 0; f < 2; f++) {
        int A;
        uint32_t val;
        int32_t key;
        bool has = valid;
        if (op == SP_LEAD) {                                   // refinement.c:210-220
            A = f ? BA_L : BA_E;
            val = f ? v.x : v.w + 1u;
            key = (int32_t)v.x;
        } else if (op == OP_INS) {                             // :299
            A = BA_I;
            val = v.x;
            key = (int32_t)v.z;
            has = has && f == 0;
        } else if (op == SP_TRAIL) {                           // :147-159
            A = BA_S;
            val = v.x;
            key = (int32_t)min(v.x, v.z);
            has = has && f == 0;
        } else {                                               // D > 50: :124, :188
            A = f ? BA_E : BA_S;
            val = f ? v.x + (v.y >> 4) + 1u : v.x;
            key = (int32_t)v.z;
        }
        const uint32_t gg = min(val >> BKS, nbt - 1u);         // (< 2^22: a contig's buckets)
        const uint32_t kk = (uint32_t)A << 28 | gg;
        const uint64_t g = (uint64_t)A * (b.nbk + 1) + cb + gg;
        uint32_t *cur = b.cur;
        uint32_t o0 = 0, n = 0;
        if (!COUNT && has) {   // (in flight while the slots are taken)
            o0 = b.off[g];
            n = b.off[g + 1] - o0;
        }
#if SVT_BK_AGG == 0
        if (!COUNT) {   // one atomic per lane, the wave's in one instruction (a single round trip)
            if (has) {
                const uint32_t sl = atomicAdd(&cur[g], 1u) - b.k * n;
                if (sl >= n) *b.err = 3u;
                else b.ev[o0 + sl] = v;
            }
            continue;
        }
#endif
        // group the lanes by bucket (lowest lane of each group: its leader, holding the group's
        // size); the leaders' atomics go out together after the loop, one round trip for all
        uint32_t rank = 0, gsz = 0;
        int lead = 0;
        for (uint64_t rem = ballot(has); rem;) {
            const int l = __builtin_ctzll(rem);
            const uint32_t kl = rdlane(kk, l);
            const uint64_t m = ballot(has && kk == kl);
            if (COUNT) {   // the bucket's count, and its BELOW key's maximum over the group
                int32_t km = (m >> ln) & 1ull ? key : -1;
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) km = max(km, __shfl_xor(km, d, WAVE));
                if (ln == l) {
                    atomicAdd(&cur[g], (uint32_t)__popcll(m));
                    if (A < 3) atomicMax(&b.pmx[g], km);
                }
            }
            if ((m >> ln) & 1ull) {
                lead = l;
                rank = mbcnt(m);
                gsz = (uint32_t)__popcll(m);
            }
            rem &= ~m;
        }
        if (COUNT) continue;
        uint32_t got = 0;
        if (has && lead == ln) got = atomicAdd(&cur[g], gsz);
        const uint32_t base = (uint32_t)__shfl((int)got, lead, WAVE);
        if (has) {
            const uint32_t sl = base - b.k * n + rank;
            if (sl >= n) *b.err = 3u;
            else b.ev[o0 + sl] = v;
        }
    }
}

// The filing of event v (0 or 1: its two filings; a D > 50 op and a leading S have two, the others
// one): array, value.
__device__ __forceinline__ bool bk_filing(const uint4 &v, int f, int &A, uint32_t &val) {
    const uint32_t op = v.y & 0xfu;
    if (op == SP_LEAD) { A = f ? BA_L : BA_E; val = f ? v.x : v.w + 1u; return true; }   // refinement.c:210-220
    if (op == OP_INS) { A = BA_I; val = v.x; return f == 0; }                              // :299
    if (op == SP_TRAIL) { A = BA_S; val = v.x; return f == 0; }                            // :147-159
    A = f ? BA_E : BA_S;                                                                   // D > 50: :124, :188
    val = f ? v.x + (v.y >> 4) + 1u : v.x;
    return true;
}

// Short reads, filing pass: a lane per read walks its CIGAR straight from the stream (rec.w = the
// read's contig) and stages the group's events in LDS.  Each filing takes its rank among the group's
// filings of its bucket from an LDS counter (the group's buckets lie within BKG_W buckets of its
// first read's bucket: reads of ~15 kb starting within ~32 kb); then one global atomic per (array,
// bucket) of the group reserves the bucket's slots for all of them, and each filing's slot is that
// base + its rank.  Same-address atomics serialise in the L2, and one locus's events come from
// neighbouring reads -- the same group: one atomic per event took 2.08 ms on cfg4, grouping the
// wave's lanes by bucket with a ballot loop 1.28 ms (profiles/r06_G, r06_H).  Filings outside the
// group's LDS window, events past the stage and groups spanning two contigs take one global atomic
// each (bk_event).
constexpr uint32_t BKG_W = 64;   // buckets per array a group counts in LDS
static_assert(BA_N * BKG_W == 4 * WAVE, "the scan below takes four counters a lane");
// The stage holds an event in 9 B (its walk position, its op word, its read's lane: the read's
// start, end and walk end are per lane), so it holds every group of cfg4 (170 events on average,
// 228 at the 99.9th percentile) within 5.5 KB a wave.  A 16-B stage of 176 events overflowed in 38 %
// of cfg4's groups (3 % of the events took a global atomic each).
#ifndef SVT_IXB_EVCAP
#define SVT_IXB_EVCAP 256
#endif
#ifndef SVT_IXB_SORT
#define SVT_IXB_SORT 0   // 1: the counted filings sorted by bucket in LDS first (coalesced stores; no faster: profiles/r06_X)
#endif
#ifndef SVT_IXB_WPB
#define SVT_IXB_WPB 2
#endif
constexpr uint32_t IXB_EVCAP = SVT_IXB_EVCAP;
constexpr int IXB_WPB = SVT_IXB_WPB;   // waves (groups) per workgroup of the filing pass
#ifndef SVT_IXB_U
#define SVT_IXB_U 4
#endif
constexpr int IXB_U = SVT_IXB_U;       // 16-B stream loads per lane per walk step (4: 16 ops, 70 VGPRs, 7 waves/SIMD; 8: 120 VGPRs, 2: 50 -- both slower, profiles/r06_V)
static_assert(IXB_EVCAP <= 0x8000u && IXB_EVCAP % WAVE == 0, "srt's 15-bit event field; whole rows of ranks");
struct BkgLds {
    uint32_t ex[IXB_EVCAP];       // the group's events: walk position (the event's x)
    uint32_t ew[IXB_EVCAP];       //   op word (or SP_TRAIL / SP_LEAD)
    uint8_t el[IXB_EVCAP];        //   the read's lane
    uint32_t rp[WAVE], re[WAVE], rw[WAVE];   // per read: start, end, walk end
    uint32_t cnt[BA_N][BKG_W];    // per bucket of the window: filings, then the group's base slot
    union {                       // one after the other in a group's life:
        uint32_t rk[IXB_EVCAP];   //   the filings' ranks in the group's buckets (f0 | f1 << 16; 0xffff: global)
        uint16_t srt[2 * IXB_EVCAP];   // the counted filings bucket by bucket: event | filing << 15
        int32_t kmx[3 * BKG_W];   //   (counting pass) the BELOW-key maxima per bucket
    };
    uint16_t loc[BA_N * BKG_W];   // the buckets' first filing in srt (exclusive scan of cnt)
};
// A staged event as the index holds it: {x, word, read end, read start} ({x, SP_LEAD, read end,
// walk end} for a leading S: svt_index2.inc's ix2_emit_read)
__device__ __forceinline__ uint4 bkg_event(const BkgLds &L, uint32_t i) {
    const uint32_t l = L.el[i], w = L.ew[i];
    return make_uint4(L.ex[i], w, L.re[l], w == SP_LEAD ? L.rw[l] : L.rp[l]);
}
// The lanes' slots for cnt (< 64) events each, in lane order after the wave's nst staged ones; nst
// advances by the wave's total.  Every lane of the wave runs it (ballots of cnt's bits).
__device__ __forceinline__ uint32_t bkg_reserve(uint32_t cnt, uint32_t &nst) {
    uint32_t x = 0, t = 0;
#pragma unroll
    for (int bt = 0; bt < 6; bt++) {
        const uint64_t m = ballot((cnt >> bt) & 1u);
        x += mbcnt(m) << bt;
        t += (uint32_t)__popcll(m) << bt;
    }
    const uint32_t s = nst + x;
    nst += t;
    return s;
}
// Each filing's rank among the group's filings of its bucket (f0 | f1 << 16; 0xffff: outside the
// LDS window).  Only the event's x, word and (leading S) walk end are read.
__device__ __forceinline__ uint32_t bkg_rank(BkgLds &L, const uint4 &v, uint32_t nbt, uint32_t gmin) {
    uint32_t rk = 0;
#pragma unroll
    for (int f = 0; f < 2; f++) {
        int A;
        uint32_t val;
        uint32_t q = 0xffffu;
        if (bk_filing(v, f, A, val)) {
            const uint32_t w = min(val >> BKS, nbt - 1u) - gmin;   // (values >= the group's first pos)
            if (w < BKG_W) q = atomicAdd(&L.cnt[0][0] + (uint32_t)A * BKG_W + w, 1u);
        }
        rk |= min(q, 0xffffu) << (16 * f);
    }
    return rk;
}
template <bool COUNT>
__global__ __launch_bounds__(64 * IXB_WPB) void ixb_lane_kernel(IxArgs a, BkBuild b, uint64_t n_reads) {
    __shared__ BkgLds lds_all[IXB_WPB];
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int ln = lane_id();
    const uint64_t g0 = ((uint64_t)blockIdx.x * IXB_WPB + wid) * WAVE;
    if (g0 >= n_reads) return;
    BkgLds &L = lds_all[wid];
    const uint64_t r = g0 + (uint64_t)ln;
    const bool act = r < n_reads;
    const uint4 rc = act ? a.rec[r] : make_uint4(0, 0, 0, 0);
    const uint64_t s = act ? a.soff[r] : 0ull, e = act ? a.soff[r + 1] : 0ull;
    const uint32_t tid = act ? rc.w : 0u, pos = rc.x, endp = rc.y, clip = rc.z >> 30;
    const uint32_t t0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)tid);   // lane 0 always holds a read
    const bool stage = ballot(act && tid != t0) == 0ull;                      // one contig: staged filing
    const uint64_t cb = b.cbase[t0];
    const uint32_t nbt = b.cnb[t0];
    const uint32_t gmin = min((uint32_t)__builtin_amdgcn_readfirstlane((int)pos) >> BKS, nbt - 1u);   // reads sorted by pos
    for (uint32_t i = (uint32_t)ln; i < BA_N * BKG_W; i += WAVE) (&L.cnt[0][0])[i] = 0u;
    uint32_t maxd = 0;   // (COUNT: the lane's longest D > 50)
    // the walk (refinement.c:118-159 / :184-221 / :295-318, the reference's per-read loop done once
    // per read), IXB_U vectors of 4 ops a step: the step's event flags first, one reservation for the
    // lane's events of the step, then the walk positions and the events into their slots.  Every lane
    // runs every step (the ballots); a lane past its read has no words.  GLOBAL: the same walk again
    // (the same slots), filing on their own the events that did not fit the stage (or all of them, in
    // a group of two contigs) -- off the common path, which holds no global atomics
    const uint4 *S4 = reinterpret_cast<const uint4 *>(a.stream);
    const uint64_t v0 = s & ~3ull;
    const uint32_t lead = (uint32_t)(s - v0), nops = (uint32_t)(e - s), span = act ? lead + nops : 0u;
    auto walk = [&](auto global_) -> uint32_t {
        constexpr bool GLOBAL = decltype(global_)::value;
        uint32_t nst = 0;   // the wave's events so far (wave-uniform)
        auto put = [&](uint32_t sl, uint32_t x, uint32_t w, uint32_t wend) {
            const bool st = stage && sl < IXB_EVCAP;
            if (!GLOBAL) {
                if (COUNT && (w & 0xfu) == OP_DEL) maxd = max(maxd, w >> 4);
                if (st) {
                    L.ex[sl] = x;
                    L.ew[sl] = w;
                    L.el[sl] = (uint8_t)ln;
                }
            } else if (!st) {
                bk_event<COUNT>(b, tid, pos, make_uint4(x, w, endp, w == SP_LEAD ? wend : pos));
            }
        };
        uint32_t cur = min(pos, IX_SAT);   // refinement.c:118's reference_pos
        for (uint32_t o = 0; ballot(o < span); o += 4 * IXB_U) {
            uint32_t w[4 * IXB_U];
#pragma unroll
            for (int u = 0; u < IXB_U; u++) {
                const uint4 q = o + 4u * u < span ? S4[(v0 >> 2) + (o >> 2) + u] : make_uint4(0, 0, 0, 0);
                w[4 * u] = q.x, w[4 * u + 1] = q.y, w[4 * u + 2] = q.z, w[4 * u + 3] = q.w;
            }
            uint32_t fl = 0;
#pragma unroll
            for (int j = 0; j < 4 * IXB_U; j++) {
                const uint32_t jr = o + (uint32_t)j - lead;   // the op's index in the read (wraps before it)
                w[j] = jr < nops ? w[j] : 0u;                 // (a 0 word: 0M, no advance)
                fl |= (ix_isD(w[j]) || ix_isI(w[j])) ? 1u << j : 0u;
            }
            uint32_t sl = bkg_reserve((uint32_t)__popc(fl), nst);
#pragma unroll
            for (int j = 0; j < 4 * IXB_U; j++) {
                if ((fl >> j) & 1u) put(sl++, cur, w[j], 0u);   // :124, :188, :299
                cur = min(cur + ref_adv(w[j]), IX_SAT);        // :141
            }
        }
        // the clip markers after the read's last op
        const bool tr = clip & SVT_CLIP_LAST_S, ld = clip & SVT_CLIP_FIRST_S;
        uint32_t sl = bkg_reserve((uint32_t)tr + (uint32_t)ld, nst);
        if (tr) put(sl++, cur, SP_TRAIL, 0u);    // :120, :147
        if (ld) put(sl++, pos, SP_LEAD, cur);    // :210
        if (!GLOBAL) L.rw[ln] = cur;
        return nst;
    };
    const uint32_t nst = walk(std::false_type{});
    if (!stage || nst > IXB_EVCAP) walk(std::true_type{});
    L.rp[ln] = pos;
    L.re[ln] = endp;
    if (COUNT) {   // the contig's longest D > 50: one atomic per wave for a one-contig group (a
                   // same-address atomic from every lane of every wave serialised: 44 ms at load on cfg4)
        if (stage) {
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) maxd = max(maxd, (uint32_t)__shfl_xor((int)maxd, d, WAVE));
            if (ln == 0 && maxd) atomicMax(&b.maxd[t0], maxd);
        } else if (act && maxd) {
            atomicMax(&b.maxd[tid], maxd);
        }
    }
    if (!stage) return;
    wave_sync();
    const uint32_t n = min(nst, IXB_EVCAP);
    if (COUNT) {   // the counting pass (load time): the group's counts and BELOW-key maxima per bucket in
                   // LDS, then one pair of global atomics per bucket
        int32_t *kmx = L.kmx;
        for (uint32_t i = (uint32_t)ln; i < 3 * BKG_W; i += WAVE) kmx[i] = -1;
        wave_sync();
        for (uint32_t i = (uint32_t)ln; i < n; i += WAVE) {
            const uint4 v = bkg_event(L, i);
#pragma unroll
            for (int f = 0; f < 2; f++) {
                int A;
                uint32_t val;
                if (!bk_filing(v, f, A, val)) continue;
                const uint32_t op = v.y & 0xfu;
                const int32_t key = op == SP_LEAD ? (int32_t)v.x : op == SP_TRAIL ? (int32_t)min(v.x, v.z) : (int32_t)v.z;
                const uint32_t w = min(val >> BKS, nbt - 1u) - gmin;
                if (w < BKG_W) {
                    atomicAdd(&L.cnt[0][0] + (uint32_t)A * BKG_W + w, 1u);
                    if (A < 3) atomicMax(kmx + (uint32_t)A * BKG_W + w, key);
                } else {
                    bk_put<true>(b, A, t0, val, v, key);
                }
            }
        }
        wave_sync();
        for (uint32_t i = (uint32_t)ln; i < BA_N * BKG_W; i += WAVE) {
            const uint32_t A = i / BKG_W, w = i % BKG_W, c = (&L.cnt[0][0])[i];
            const uint64_t g = (uint64_t)A * (b.nbk + 1) + cb + gmin + w;
            if (c) atomicAdd(&b.cur[g], c);
            if (A < 3 && kmx[i] >= 0) atomicMax(&b.pmx[g], kmx[i]);
        }
        return;
    }
    // (a pass over the stage: taking the ranks as the walk stages each event was slower, its LDS
    // atomics' returns waited on inside the walk's branches -- index 0.75 vs 0.54 ms, profiles/r06_AG)
    for (uint32_t i = (uint32_t)ln; i < n; i += WAVE) L.rk[i] = bkg_rank(L, bkg_event(L, i), nbt, gmin);
    wave_sync();
    // the group's filings bucket by bucket (a counting sort in LDS), so that the stores below go to
    // consecutive slots from consecutive lanes; the buckets' reservations, one atomic each, all in
    // flight at once
    uint32_t nf;
    {
        uint32_t c4[4], sum = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) { c4[q] = (&L.cnt[0][0])[4 * ln + q]; sum += c4[q]; }
        uint32_t tot;
        uint32_t x = wave_excl(sum, tot);
        nf = tot;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t i = 4u * (uint32_t)ln + (uint32_t)q, A = i / BKG_W, w = i % BKG_W;
            L.loc[i] = (uint16_t)x;
            x += c4[q];
            if (c4[q]) {   // the bucket's extent loaded beside its reservation: cnt = the group's first slot
                const uint64_t g = (uint64_t)A * (b.nbk + 1) + cb + gmin + w;
                const uint32_t o0 = b.off[g], nb = b.off[g + 1] - o0;
                const uint32_t sl = atomicAdd(&b.cur[g], c4[q]) - b.k * nb;
                if (sl > nb || c4[q] > nb - sl) *b.err = 3u;
                (&L.cnt[0][0])[i] = o0 + sl;
            }
        }
    }
    // srt shares rk's words: every lane takes its ranks into registers first
    constexpr int RKL = IXB_EVCAP / WAVE;
    uint32_t rkl[RKL];
#pragma unroll
    for (int k = 0; k < RKL; k++) {
        const uint32_t i = (uint32_t)ln + (uint32_t)k * WAVE;
        rkl[k] = i < n ? L.rk[i] : 0u;
    }
    wave_sync();
#pragma unroll
    for (int k = 0; k < RKL; k++) {
        const uint32_t i = (uint32_t)ln + (uint32_t)k * WAVE;
        if (i >= n) break;
        const uint4 v = bkg_event(L, i);
        const uint32_t rk = rkl[k];
#pragma unroll
        for (int f = 0; f < 2; f++) {
            int A;
            uint32_t val;
            if (!bk_filing(v, f, A, val)) continue;
            const uint32_t q = (rk >> (16 * f)) & 0xffffu;
            const uint32_t gg = min(val >> BKS, nbt - 1u);
            if (q != 0xffffu && SVT_IXB_SORT) {   // counted: its place in srt
                L.srt[L.loc[(uint32_t)A * BKG_W + gg - gmin] + q] = (uint16_t)(i | (uint32_t)f << 15);
                continue;
            }
            if (q != 0xffffu) {   // (unsorted: straight to its slot)
                const uint32_t at = (&L.cnt[0][0])[(uint32_t)A * BKG_W + gg - gmin] + q;
                if (at < b.n_ev) b.ev[at] = v;
                continue;
            }
            const uint64_t g = (uint64_t)A * (b.nbk + 1) + cb + gg;   // outside the window: its own atomic
            const uint32_t o0 = b.off[g], nb = b.off[g + 1] - o0;
            const uint32_t sl = atomicAdd(&b.cur[g], 1u) - b.k * nb;
            if (sl >= nb) *b.err = 3u;
            else b.ev[o0 + sl] = v;
        }
    }
    if (!SVT_IXB_SORT) return;
    wave_sync();
    for (uint32_t j = (uint32_t)ln; j < nf; j += WAVE) {
        const uint32_t e = L.srt[j], i = e & 0x7fffu;
        const uint4 v = bkg_event(L, i);
        int A;
        uint32_t val;
        bk_filing(v, (int)(e >> 15), A, val);
        const uint32_t wi = (uint32_t)A * BKG_W + min(val >> BKS, nbt - 1u) - gmin;
        const uint32_t at = (&L.cnt[0][0])[wi] + (j - L.loc[wi]);   // (checked against the extent above)
        if (at < b.n_ev) b.ev[at] = v;
    }
}

// The captured builds' cursors zeroed (a kernel node: a captured hipMemsetAsync of this size did not
// re-zero them at every replay -- the second replay's events fell outside their extents).
__global__ __launch_bounds__(256) void bk_zero_kernel(uint4 *p, uint64_t n4) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (uint64_t)gridDim.x * 256) p[i] = make_uint4(0, 0, 0, 0);
}

// Long reads: the span lists (rebuilt first by the stream walk) filed, a lane per read, the wave's
// j-th events together (bk_file_wave) when its reads lie in one contig.
constexpr int IXB_T = 256;
template <bool COUNT>
__global__ __launch_bounds__(IXB_T) void ixb_lists_kernel(IxArgs a, BkBuild b, uint64_t n_reads) {
    const uint64_t r = (uint64_t)blockIdx.x * IXB_T + threadIdx.x;
    const uint64_t w0 = r - (uint64_t)lane_id();
    if (w0 >= n_reads) return;
    const bool act = r < n_reads;
    const uint4 rc = act ? a.rec[r] : make_uint4(0, 0, 0, 0);
    const uint32_t t0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)rc.w);
    const bool one = ballot(act && rc.w != t0) == 0ull;
    uint32_t maxd = 0;   // (COUNT: the lane's longest D > 50)
    for (int q = 0; q < 2; q++) {
        const uint64_t *so = q ? a.spoffI : a.spoffD;
        const uint4 *sp = q ? a.spI : a.spD;
        const uint64_t e0 = act ? so[r] : 0ull, e1 = act ? so[r + 1] : 0ull;
        if (!one) {
            for (uint64_t i = e0; i < e1; i++) bk_event<COUNT>(b, rc.w, rc.x, sp[i]);
            continue;
        }
        uint32_t nmax = (uint32_t)(e1 - e0);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) nmax = max(nmax, (uint32_t)__shfl_xor((int)nmax, d, WAVE));
        const uint64_t cb = b.cbase[t0];
        const uint32_t nbt = b.cnb[t0];
        for (uint32_t j = 0; j < nmax; j++) {
            const bool h = e0 + j < e1;
            uint4 v = h ? sp[e0 + j] : make_uint4(0, 0, 0, 0);
            if (h && v.y != SP_LEAD) v.w = rc.x;
            if (COUNT && h && (v.y & 0xfu) == OP_DEL) maxd = max(maxd, v.y >> 4);
            bk_file_wave<COUNT>(b, cb, nbt, v, h);
        }
    }
    if (COUNT) {   // one atomic per wave: same-address atomics from every lane serialise
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) maxd = max(maxd, (uint32_t)__shfl_xor((int)maxd, d, WAVE));
        if (lane_id() == 0 && maxd) atomicMax(&b.maxd[t0], maxd);
    }
}

// Long reads, filing pass: the stream walk (index_kernel) staged every range's events in its scratch
// slot; a wave files one range's events from there, 64 at a time (bk_file_wave) -- no span lists,
// no scan of the range totals in the step.  A range whose events overflowed its stage is walked
// again, filing straight from the walk (ix_range<IXM_BUCKET>).  A range lies in one contig.
__global__ __launch_bounds__(64 * IX_WPB) SVT_IXC_OCC void ixb_copy_kernel(IxArgs a, BkBuild b) {
    __shared__ IxEmitLds lds_all[IX_WPB];
    __shared__ IxStage stg_all[IX_WPB];
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t w = blockIdx.x * IX_WPB + wid;
    if (w >= a.n_ranges) return;
    const int ln = lane_id();
    if (uniform_i((int)a.ovf[w])) {
        bool unused = false;
        uint64_t bD = 0, bI = 0;
        ix_range<IXM_BUCKET>(a, w, lds_all[wid], stg_all[wid], bD, bI, unused, &b);
        return;
    }
    const uint64_t ra = rdlane64(a.part[w], 0);
    const uint32_t t0 = rdlane(a.rec[ra].w, 0);
    const uint64_t cb = b.cbase[t0];
    const uint32_t nbt = b.cnb[t0];
    const uint32_t nD = (uint32_t)rdlane64(a.agg[w].v[IX_D], 0), nI = (uint32_t)rdlane64(a.agg[w].v[IX_I], 0);
    const uint4 *ev = a.scr + (uint64_t)w * IX_SCAP;
    for (uint32_t i0 = 0; i0 < nD + nI; i0 += WAVE) {
        const uint32_t i = i0 + (uint32_t)ln;
        const bool h = i < nD + nI;
        const uint4 v = h ? ev[i < nD ? i : IX_SCAP - 1u - (i - nD)] : make_uint4(0, 0, 0, 0);
        bk_file_wave<false>(b, cb, nbt, v, h);
    }
}
