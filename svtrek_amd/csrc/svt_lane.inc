// svt_lane.inc -- refine_lane_kernel, the default timed kernel, and its helpers (included by
// svt_engine.hip after svt_refine.inc).

// ------------------------------------------------------------------ lane-vote kernel
// The default timed kernel.  A wave takes LV_W consecutive windows.  Phase 1, per window
// and wave-wide: the A2 window, the span query and walk (A3-A7) and the exact band filter
// (band_filter); a window whose band holds <= LV_CAP elements, all >= 0, within +-1023 of
// pos (the common case: ~20 candidates of its own breakpoint) is staged in LDS as 16-bit
// offsets from the band's low end, with the band's three whole-multiset facts.  Phase 2,
// one LANE per staged window: an in-register sorting network over the lane's offsets,
// 16-bit prefix sums, and consensus_pos (refinement.c:41-101) run per lane as the
// reference's own loops -- with the cluster starts/ends as two pointers that only move
// one way along a pass -- so the sort and the vote cost a few instructions per window
// instead of a wave-wide network and per-lane searches for every window.  Phase 3: the
// other windows (band off, > LV_CAP band elements, > CAP candidates) are re-gathered and
// voted wave-wide (refine_window), as refine_span_kernel does.  Same results.
// Windows per wave (<= 64: one lane each in phase 2): 64, so that the sort network and the
// vote's loops issue with every lane at work -- taken through phases 0-1 in two rounds of 32,
// which keeps the win table and so the wave's LDS small (7 waves per SIMD) -- or 32 for
// launches too small to fill the chip with 64 per wave (svt_ctx::launch).
constexpr int LV_CAP = 32;   // band elements a lane votes on
constexpr int LV_S = 34;     // u16 per staged row (17 words: odd -> no bank conflicts)
static_assert(LV_S > LV_CAP, "a staged row needs a spare slot past LV_CAP");
// refine_lane_kernel: phases 0-1 take LV_R windows a round.  Its waves per SIMD follow from the
// windows per wave: at 64 the wave's LDS (LaneLds<64>: 5 632 B a wave) allows 7 workgroups a CU, so
// 7; at 32 (3 968 B) the refine kernels' 8.
constexpr int LV_R = 32;
constexpr int lane_waves(int lv_w) { return lv_w == 64 ? 7 : REFINE_WAVES; }
// Windows a launch needs for 64 per wave (svt_ctx::launch): the 250K-window launch of a 125K-locus
// shard is the smallest measured, and 64 per wave wins there (0.118 vs 0.127 ms a step at 32,
// profiles/e0260); smaller launches keep 32 per wave.
constexpr size_t LANE_WIDE_MIN = 250000;
// LV_BELOW / LV_ABOVE: some candidate lies at or below the band's low end / at or above its high
// end (with the band itself they give band_filter's whole-multiset facts, see lane_vote)
constexpr uint32_t LV_PENDING = 1u << 8, LV_BELOW = 1u << 9, LV_ABOVE = 1u << 10,
                   LV_REDO = 1u << 13;

// A window's flags word (LaneLds::flags): nb | LV_* bits.  It is the only per-window fact another
// lane writes in phase 1; the band's low end stays in the owning lane's registers.
constexpr uint32_t LV_NONE = 1u << 14;   // no window (INV / other types): NA

// Phase 1's packed walk: the windows with a span to walk, in wave order, one entry
// each (written by their phase-0 lanes); consecutive windows of <= 64 events together share
// one 64-event slot.
// (24 B: the band's low end is not kept -- lv_lo gives it back from s and the kind -- so that
// the wide kernel's LDS leaves room for 6-7 waves per SIMD.)
constexpr uint32_t LVW_BELOW = 1u << 16;
struct alignas(8) LvWin {
    uint64_t e0;    // the span's first event
    uint32_t s, e;  // the window
    uint32_t kl;    // kind | the window's row << 8 | LVW_BELOW (value buckets: the prefix maxima below
                    // the band's buckets hold a candidate)
    uint32_t len;   // span events (> 0)
};
// The band's low end pos - (range + max(ci, 0)) from the window's start: s = pos - wider / median /
// narrow in uint32 (window_of), so s + that width is pos again, bit for bit.
__device__ __forceinline__ int32_t lv_lo(const KParams &k, uint32_t kind, uint32_t s, int32_t bw) {
    const int32_t d = kind == (uint32_t)K_INS ? k.median : kind == (uint32_t)K_START ? k.wider : k.narrow;
    return (int32_t)(s + (uint32_t)d) - bw;
}

// W rows for phase 2 (one lane each), LV_R windows per round of phases 0-1 (the win table is per round).
template <int W>
struct LaneLds {
    uint16_t stage[W * LV_S];   // band offsets (phase 1 -> 2)
    uint32_t flags[W];
    LvWin win[LV_R];
    uint32_t sink[WAVE];        // lane_walk: the store target of lanes without a band member
};

// Phase 1 of one window, wave-wide (A4-A7 + the band): the window's span events [E0, E0+len)
// are tested 64 * LW_U at a time (LW_U 16-B loads per lane in flight), and each candidate goes
// straight to the exact band of consensus_pos (band_filter's rule, see there): members in
// (lo, hi) are written to the window's row as 16-bit offsets from lo, and whether any candidate
// lies at or below lo / at or above hi is accumulated per lane (with the band they give the
// whole-multiset facts, lane_vote).  Values are walk positions < 2^29 + 1 (reads reaching 2^28
// bases or position 2^29 are slow and carry no events), so every candidate is >= 0 and within
// +-2^30: no int64 path is ever needed.  refine_end's leading-S reads whose walk passes e count
// as one candidate at or above the band's high end (KParams::sent_ok).
struct LaneBand {
    int32_t nb;       // band members (> LV_CAP: the row overflowed)
    uint32_t flags;   // LV_BELOW | LV_ABOVE
};

constexpr int LW_U = 4;   // 64-event slots per step of lane_walk (loads in flight per lane)
// lane_walk reads the span through a buffer descriptor of the window's own span (wave-uniform
// base and byte count): a lane's byte offset is the constant ln * 16 (+ the slot's immediate
// offset), so a load costs no VALU address arithmetic, and a load past the span returns zeros --
// an op-0 (M) event, never a candidate -- so no clamp and no partial-slot mask either.  Spans of
// 2^27 events or more take the wave-wide path (LvQuery), so the byte count fits 32 bits.
constexpr uint32_t LW_BUF_MAX = 1u << 27;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// The min_count test (refinement.c:43) is made on the band size instead of the candidate count.
// Exact: an accepted cluster lies inside the band (its elements are within ci of an element
// within range of pos), so the vote returns -1 whenever the band holds fewer than min_count
// elements, and n < min_count implies nb < min_count.  The walk then keeps no count.

// One slot as vector arithmetic.  The kernel is bound by scalar issue (one SALU instruction per
// CU and cycle): every test is the sign bit of a difference ("fail" bits), OR-ed per lane; the
// band is one unsigned compare whose lane mask is the only ballot, and below / above accumulate
// as sign bits in VGPRs (one ballot each per window).  Exact: the operands' ranges keep every
// difference inside int32 -- walk positions and candidate values <= 2^30 + 2^28 + 1 (IX_SAT, one
// op < 2^28), endpos in [1, 2^30) (slow reads carry no events), e < 2^30 (WEXACT),
// lo >= -2^29 (lane_query), the window start clamped (LwWin).
struct LwWin {
    int32_t b1;     // max(s - 1, -2^30) + 1: the overlap test endpos > s - 1 is endpos - b1 >= 0
    uint32_t e;
    int32_t sc;     // s, or 2^31 - 1 when s >= 2^31 (a window start that wrapped: x >= s never holds)
    int32_t lo1;    // lo + 1: a value v is at or below the band when v - lo1 < 0
    int32_t hm1;    // hi - 1: at or above it when hm1 - v < 0
    uint32_t wb;    // hi - lo - 1: in the band when (uint32)(v - lo1) < wb
    int32_t em2;    // e - 2 (value buckets: the event's read is yielded when its pos <= e - 2)
};
__device__ __forceinline__ uint32_t sgn(int32_t d) { return (uint32_t)d >> 31; }
__device__ __forceinline__ uint32_t opbit(uint32_t set, uint32_t op) { return __builtin_amdgcn_ubfe(set, op, 1); }

// One 64-event slot: the band's lane mask; below / above accumulated into the sign bits of
// belv / abv; iv = the lane's candidate value.
template <int KIND, bool BK>
__device__ __forceinline__ uint64_t slot_vl(const uint4 &v, const LwWin &W, uint32_t &belv, uint32_t &abv, int32_t &iv) {
    const uint32_t op = v.y & 0xfu;
    // value buckets: the event's read must also be yielded (its pos -- v.w, v.x for a leading S --
    // below the query end); a span holds only yielded reads' events
    const uint32_t yld = BK ? sgn(W.em2 - (int32_t)v.w) : 0u;
    const uint32_t far = sgn((int32_t)v.z - W.b1) | sgn((int32_t)W.e - (int32_t)v.x) | yld;   // no overlap / not reached
    uint32_t fail;
    if (BK && KIND == K_END) {                                            // :188, :210-220
        const uint32_t isD = opbit(1u << OP_DEL, op), isL = opbit(1u << SP_LEAD, op);
        const uint32_t lead = isL & (sgn((int32_t)v.z - W.b1) ^ 1u) & (sgn((int32_t)v.x - W.sc) ^ 1u) &
                              (sgn(W.em2 - (int32_t)v.x) ^ 1u);
        const uint32_t brk = lead & sgn((int32_t)W.e - (int32_t)v.w);   // walk passes e: a value >= e + 2
        abv |= brk << 31;
        fail = ((isD & (far ^ 1u)) | (lead & (brk ^ 1u))) ^ 1u;
        iv = (int32_t)(isD ? v.x + (v.y >> 4) + 1u : v.w + 1u);
    } else if (KIND == K_INS) {                                           // refinement.c:299
        fail = far | (opbit(1u << OP_INS, op) ^ 1u);
        iv = (int32_t)v.x;
    } else if (KIND == K_START) {                                         // :124, :147
        fail = far | (opbit(1u << OP_DEL | 1u << SP_TRAIL, op) ^ 1u) |
               (opbit(1u << SP_TRAIL, op) & sgn((int32_t)v.x - W.sc));
        iv = (int32_t)v.x;
    } else {                                                              // :188, :210-220
        const uint32_t isD = opbit(1u << OP_DEL, op);
        const uint32_t lead = opbit(1u << SP_LEAD, op) & (far ^ 1u) & (sgn((int32_t)v.x - W.sc) ^ 1u);
        const uint32_t brk = lead & sgn((int32_t)W.e - (int32_t)v.w);   // walk passes e: a value >= e + 2
        abv |= brk << 31;
        fail = ((isD & (far ^ 1u)) | (lead & (brk ^ 1u))) ^ 1u;
        iv = (int32_t)(isD ? v.x + (v.y >> 4) + 1u : v.w + 1u);
    }
    const uint32_t d = (uint32_t)(iv - W.lo1);
    const uint32_t pass = (fail ^ 1u) << 31;
    belv |= d & pass;
    abv |= (uint32_t)(W.hm1 - iv) & pass;
    return ballot((d | fail << 31) < W.wb);
}

// The window's scalar inputs (base address of its span, span length, LwWin, lo, its staging
// row) come from the caller's v_readlane of per-lane values computed once per wave.  Every lane
// stores in every slot -- members to their row slot, the others to their own sink word -- so a
// slot costs no exec-mask round trip on the scalar unit.
template <int KIND, bool BK>
__device__ __forceinline__ LaneBand lane_walk(uint64_t evaddr, uint32_t len, const LwWin &W, int32_t lo, uint16_t *row,
                                              uint16_t *sink) {
    const int ln = lane_id();
    int32_t nb = 0;
    uint32_t belv = 0, abv = 0;
    for (uint32_t b = 0; b < len; b += LW_U * WAVE) {
        const uint32_t left = len - b;
        uint4 v[LW_U];
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            reinterpret_cast<void *>(evaddr + (uint64_t)b * 16u), (short)0, (int)(left * 16u), 0x00020000);
#pragma unroll
        for (int u = 0; u < LW_U; u++) {   // all four in flight at once; past the span: zeros
            const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(rs, ln * 16 + u * WAVE * 16, 0, 0);
            v[u] = make_uint4(r.x, r.y, r.z, r.w);
        }
#pragma unroll
        for (int u = 0; u < LW_U; u++) {
            if ((uint32_t)(u * WAVE) >= left) break;
            int32_t iv;
            const uint64_t mb = slot_vl<KIND, BK>(v[u], W, belv, abv, iv);
            // members past LV_CAP all land in the row's spare slot LV_CAP (the window is redone);
            // the slot is computed by every lane (the empty asm keeps the compiler from moving it
            // under a branch on the member mask), then one select
            uint32_t at = (uint32_t)min(nb + (int32_t)mbcnt(mb), LV_CAP);
            asm volatile("" : "+v"(at));
            uint16_t *dst = __builtin_amdgcn_inverse_ballot_w64(mb) ? row + at : sink;
            *dst = (uint16_t)(iv - lo);
            nb += (int32_t)__popcll(mb);
        }
    }
    const uint64_t below = ballot((int32_t)belv < 0), above = ballot((int32_t)abv < 0);
    return LaneBand{nb, (below ? LV_BELOW : 0u) | (above ? LV_ABOVE : 0u)};
}

// Two windows of the same kind with 65-128 span events each, walked together: their four slots'
// loads are in flight at once, so the pair costs one memory round trip instead of two (phase 1
// is a chain of one round trip per window per wave, ~24 a wave on cfg4).
struct LwOne {
    uint64_t base;
    uint32_t len;
    LwWin W;
    int32_t lo;
    uint16_t *row;
};
template <int KIND, bool BK>
__device__ __forceinline__ void lane_walk2(const LwOne &A, const LwOne &B, uint16_t *sink, LaneBand &ra, LaneBand &rb) {
    const int ln = lane_id();
    const __amdgpu_buffer_rsrc_t sa = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(A.base), (short)0,
                                                                        (int)(A.len * 16u), 0x00020000);
    const __amdgpu_buffer_rsrc_t sb = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(B.base), (short)0,
                                                                        (int)(B.len * 16u), 0x00020000);
    uint4 v[4];
    {
        const u32x4 r0 = __builtin_amdgcn_raw_buffer_load_b128(sa, ln * 16, 0, 0);
        const u32x4 r1 = __builtin_amdgcn_raw_buffer_load_b128(sa, ln * 16 + WAVE * 16, 0, 0);
        const u32x4 r2 = __builtin_amdgcn_raw_buffer_load_b128(sb, ln * 16, 0, 0);
        const u32x4 r3 = __builtin_amdgcn_raw_buffer_load_b128(sb, ln * 16 + WAVE * 16, 0, 0);
        v[0] = make_uint4(r0.x, r0.y, r0.z, r0.w);
        v[1] = make_uint4(r1.x, r1.y, r1.z, r1.w);
        v[2] = make_uint4(r2.x, r2.y, r2.z, r2.w);
        v[3] = make_uint4(r3.x, r3.y, r3.z, r3.w);
    }
#pragma unroll
    for (int w = 0; w < 2; w++) {
        const LwOne &O = w ? B : A;
        int32_t nb = 0;
        uint32_t belv = 0, abv = 0;
#pragma unroll
        for (int u = 0; u < 2; u++) {
            int32_t iv;
            const uint64_t mb = slot_vl<KIND, BK>(v[2 * w + u], O.W, belv, abv, iv);
            uint32_t at = (uint32_t)min(nb + (int32_t)mbcnt(mb), LV_CAP);
            asm volatile("" : "+v"(at));
            uint16_t *dst = __builtin_amdgcn_inverse_ballot_w64(mb) ? O.row + at : sink;
            *dst = (uint16_t)(iv - O.lo);
            nb += (int32_t)__popcll(mb);
        }
        const uint64_t below = ballot((int32_t)belv < 0), above = ballot((int32_t)abv < 0);
        (w ? rb : ra) = LaneBand{nb, (below ? LV_BELOW : 0u) | (above ? LV_ABOVE : 0u)};
    }
}

// One 64-event slot holding the whole spans of consecutive walkable windows win[c0..]: bit i of
// M marks the first lane of a window (bit 0 always), tot <= 64 events in all.  Lane j walks
// event j - f of the window that starts at f = the highest mark <= j, with that window's own
// s / e / band (the tests of span_cand_mask, per lane); members go to the window's row at
// their rank among its members, and each window's first lane writes its flags word (band size,
// below / above) -- everything lane_walk gives a window, for 1-64 events at once.
// The event lane ln tests in the packed slot of windows win[c0..] with marks M (value buckets: one
// event array) -- loaded ahead of the slot's tests so that a run of packed slots keeps the next
// slot's loads in flight while the current one is tested.
__device__ __forceinline__ uint4 lane_packed_load(const BkIndex &B, const LvWin *win, uint32_t c0, uint64_t M) {
    const int ln = lane_id();
    const uint64_t upto = M & ((2ull << ln) - 1ull);
    const uint32_t r = (uint32_t)__popcll(upto) - 1u, f = 63u - (uint32_t)__clzll(upto);
    const LvWin &w = win[c0 + r];
    return B.ev[w.e0 + min((uint32_t)ln - f, w.len - 1u)];
}

template <bool BK>
__device__ __forceinline__ void lane_packed(const DevPileup &P, const BkIndex &B, const KParams &prm, const LvWin *win,
                                            uint32_t *flags, uint16_t *stage, uint32_t c0, uint64_t M, uint32_t tot,
                                            int32_t bw2, const uint4 *vpre = nullptr) {
    const int ln = lane_id();
    const uint64_t upto = M & ((2ull << ln) - 1ull);   // marks at or below this lane (ln 63: all)
    const uint32_t r = (uint32_t)__popcll(upto) - 1u, f = 63u - (uint32_t)__clzll(upto);
    const LvWin w = win[c0 + r];
    const uint32_t kind = w.kl & 0xffu, k = (w.kl >> 8) & 0xffu;
    const uint4 *evb = (BK ? B.ev : kind == (uint32_t)K_INS ? P.spI : P.spD) + w.e0;
    const uint4 v = vpre ? *vpre : evb[min((uint32_t)ln - f, w.len - 1u)];   // lanes past tot: their window's last event
    const uint32_t s = w.s, e = w.e, x = v.x, op = v.y & 0xfu;
    const int32_t lo = lv_lo(prm, kind, s, bw2 >> 1);
    const uint64_t isI = ballot(kind == (uint32_t)K_INS), isE = ballot(kind == (uint32_t)K_END);
    const uint64_t oD = ballot(op == OP_DEL), sx = ballot(s <= x), oL = ballot(op == SP_LEAD);
    const uint64_t ovl = ballot((int32_t)v.z > (int32_t)(s - 1u));
    // value buckets: the event's read is yielded (pos < e - 1: v.w, or v.x for a leading S)
    const uint64_t yw = BK ? ballot(v.w + 2u <= e) : ~0ull, yx = BK ? ballot(x + 2u <= e) : ~0ull;
    const uint64_t base = ballot((uint32_t)ln < tot) & ovl & ballot(x <= e) & (yw | (isE & oL));
    const uint64_t lead = ballot((uint32_t)ln < tot) & ovl & isE & oL & sx & (BK ? yx : ballot(x <= e));   // :210-220
    const uint64_t brk = lead & ballot(v.w > e);
    const uint64_t cm = (base & ((isI & ballot(op == OP_INS)) | (~(isI | isE) & (oD | (ballot(op == SP_TRAIL) & sx))) |
                                 (isE & oD))) |
                        (lead & ~brk);
    const int32_t iv = (int32_t)(kind == (uint32_t)K_END ? (op == OP_DEL ? x + (v.y >> 4) + 1u : v.w + 1u) : x);
    const uint64_t gt = ballot(iv > lo), lt = ballot(iv < lo + bw2);
    const uint64_t mb = cm & gt & lt;
    if ((mb >> ln) & 1ull) {
        const uint32_t rank = mbcnt(mb) - (uint32_t)__popcll(mb & ((1ull << f) - 1ull));
        stage[k * LV_S + min(rank, (uint32_t)LV_CAP)] = (uint16_t)(iv - lo);
    }
    if ((M >> ln) & 1ull) {   // the window's first lane: its totals over lanes [ln, ln + len)
        const uint64_t rm = (w.len >= 64u ? ~0ull : ((1ull << w.len) - 1ull)) << ln;
        const uint32_t nb = (uint32_t)__popcll(mb & rm);
        const bool below = (cm & ~gt & rm) != 0ull, above = ((brk | (cm & ~lt)) & rm) != 0ull;
        flags[k] = nb > (uint32_t)LV_CAP ? LV_REDO
                                         : nb | LV_PENDING | (below || (w.kl & LVW_BELOW) ? LV_BELOW : 0u) |
                                               (above ? LV_ABOVE : 0u);
    }
}

// Phase 0 fills every window's band slots with 0xffff, so phase 2 takes its band straight from
// the row (no per-slot test against the band size).  The band is sorted by Batcher's odd-even
// merge sort (19 / 63 / 191 compare-exchanges for 8 / 16 / 32 elements against 24 / 80 / 240 for
// the bitonic network, all ascending).
__device__ __forceinline__ void lv_cx(uint32_t (&x)[LV_CAP], int i, int j) {
    const uint32_t p = x[i], q = x[j];
    x[i] = min(p, q);
    x[j] = max(p, q);
}
template <int LO, int N, int R>
__device__ __forceinline__ void lv_oe_merge(uint32_t (&x)[LV_CAP]) {
    if constexpr (2 * R < N) {
        lv_oe_merge<LO, N, 2 * R>(x);
        lv_oe_merge<LO + R, N, 2 * R>(x);
#pragma unroll
        for (int i = LO + R; i + R < LO + N; i += 2 * R) lv_cx(x, i, i + R);
    } else {
        lv_cx(x, LO, LO + R);
    }
}
template <int LO, int N>
__device__ __forceinline__ void lv_oe_sort(uint32_t (&x)[LV_CAP]) {
    if constexpr (N > 1) {
        lv_oe_sort<LO, N / 2>(x);
        lv_oe_sort<LO + N / 2, N / 2>(x);
        lv_oe_merge<LO, N, 1>(x);
    }
}

// floor(x / c) for x < 2^17, 1 <= c <= 64: ((x + 1/2) * rcp(c)) lies at least 1/(2c) >= 2^-7
// inside [q, q+1) exactly, and the f32 product is within 2^-9 of it (x + 1/2 < 2^17,
// v_rcp_f32 within 1 ulp), so the truncation is exact.
__device__ __forceinline__ uint32_t div_small(uint32_t x, uint32_t c) {
    return (uint32_t)(((float)x + 0.5f) * __builtin_amdgcn_rcpf((float)c));
}

// consensus_pos (refinement.c:41-101) for one lane's staged window: B[0..nb) its band's
// sorted offsets (value - lo), w = pos - lo.  Every band value is >= 0, so the reference's
// rounded uint64 mean of a cluster is lo + (offset sum + c/2) / c.  The clusters are sliding
// windows whose ends only move one way along each pass, so their sums are kept up to date
// element by element (no prefix array).
__device__ __forceinline__ int32_t lane_vote(const uint16_t *B, int32_t nb, int32_t w, int32_t lo, uint32_t fl,
                                             const KParams &k, int32_t l0 = -1) {
    const int32_t ci = k.ci, range = k.range;
    int32_t valL = -1, maxL = k.min_count - 1, distL = 0x7fffffff;
    int32_t valR = -1, maxR = k.min_count - 1, distR = 0x7fffffff;
    // lower_bound(pos+25) over the band (refinement.c:3-10), started where the full pass would
    // (l0 >= 0: the caller counted the band elements <= pos+25 already)
    if (l0 < 0) {
        int32_t h0 = nb;
        l0 = 0;
        while (l0 < h0) {
            const int32_t md = (l0 + h0) >> 1;
            if ((int32_t)B[md] > w + SV_MIN_LENGTH / 2) h0 = md; else l0 = md + 1;
        }
    }
    // band_filter's whole-multiset facts: the band's own elements (B[0] its minimum) plus
    // whether candidates lie below / above it
    const bool below = fl & LV_BELOW, above = fl & LV_ABOVE;
    const bool u0 = !below && l0 == 0;                                          // none <= pos+25
    const bool lt = below || (nb > 0 && (int32_t)B[0] < w - SV_MIN_LENGTH / 2);   // some < pos-25
    int32_t p = u0 ? 0 : l0 == 0 ? -1 : l0 - 1;
    if (nb == 0) p = -1;
    int32_t kk = p + 1, prev = 0;   // cluster [kk, i] below i, its offset sum S
    uint32_t S = 0;
    for (int32_t i = p; i >= 0; i--) {                                       // refinement.c:58
        const int32_t a = B[i];
        if (ref_abs(w - a) >= range) break;
        if (i < p) S -= (uint32_t)prev;                                      // element i+1 leaves
        if (kk > i) { kk = i; S = (uint32_t)a; }
        while (kk > 0 && (int32_t)B[kk - 1] >= a - ci) { kk--; S += B[kk]; }   // :61-64
        prev = a;
        const int32_t c = i - kk + 1;
        if (c > maxL) {                                                      // :67-76
            const int32_t co = (int32_t)div_small(S + (uint32_t)(c / 2), (uint32_t)c);   // :65
            const int32_t d = ref_abs(w - co);
            if (d < ci) return lo + co;
            if (d < distL) { maxL = c; valL = lo + co; distL = d; }
        }
    }
    // upper_bound(pos-25) (refinement.c:12-19): the full multiset's A[0] / A[n-1]
    const int32_t q = lt ? (!below ? 0 : nb) : (!above ? nb - 1 : nb);
    int32_t m = q;   // cluster [i, m) above i
    S = 0;
    for (int32_t i = q; i < nb; i++) {                                       // :80
        const int32_t a = B[i];
        if (ref_abs(w - a) >= range) break;
        if (i > q) S -= (uint32_t)prev;                                      // element i-1 leaves
        if (m <= i) { m = i + 1; S = (uint32_t)a; }
        while (m < nb && (int32_t)B[m] <= a + ci) { S += B[m]; m++; }        // :83-86
        prev = a;
        const int32_t c = m - i;
        if (c > maxR) {                                                      // :88-97
            const int32_t co = (int32_t)div_small(S + (uint32_t)(c / 2), (uint32_t)c);   // :87
            const int32_t d = ref_abs(w - co);
            if (d < ci) return lo + co;
            if (d < distR) { maxR = c; valR = lo + co; distR = d; }
        }
    }
    return distL < distR ? valL : valR;                                      // :100
}

// One window's A2 + A3 answer, computed by one lane (phase 0).  u32 words only (the rows
// it is parked in are 4-byte aligned).
constexpr int32_t LQ_REDO = 1 << 4;   // kind bit: the window takes the wave-wide path
struct LvQuery {
    int32_t kind;          // K_* (| LQ_REDO), -1: no window (NA)
    int32_t lo;            // the vote's band low end: pos - (range + max(ci, 0))
    uint32_t s, e, liw, len;        // the window, li << 1 | w, its span's event count
    uint32_t e0[2];                 // the span's first event
    uint32_t fl;                    // value buckets: LV_BELOW from the prefix maxima
};
static_assert(sizeof(LvQuery) <= LV_S * 2, "LvQuery must fit a staging row");

__device__ __forceinline__ void lane_query(const KArgs &a, uint32_t g, bool band_ok, LvQuery &q) {
    const DevPileup &P = a.pile;
    const KParams &k = a.prm;
    const uint32_t w = g >= a.n ? 1u : 0u, li = g - w * a.n;
    const svt_locus L = a.loci[li];
    q.kind = -1;
    q.liw = li << 1 | w;
    const uint32_t pos = L.pos, end = L.end;
    uint32_t imp = 0;
    if (L.type == T_INS && w == 0) { q.kind = K_INS; q.s = pos - (uint32_t)k.median; q.e = pos + (uint32_t)k.median; imp = pos; }
    else if (L.type == T_DEL && w == 0) { q.kind = K_START; q.s = pos - (uint32_t)k.wider; q.e = pos + (uint32_t)k.narrow; imp = pos; }
    else if (L.type == T_DEL) { q.kind = K_END; q.s = end - (uint32_t)k.narrow; q.e = end + (uint32_t)k.narrow; imp = end; }
    // INV: refine_point collects only when sv_type == SV_INS (refinement.c:250): NA, NA
    if (q.kind < 0) return;
    // the wave-wide path (refine_redo_kernel) when the window ends at or past WEXACT or is a
    // refine_end window whose stops need the per-read replay (gather_span), when the band is off
    // (band_ok) or pos is beyond +-2^30 (int32 differences could wrap)
    constexpr int32_t LIM = 1 << 30;
    if (q.e >= WEXACT || (q.kind == K_END && !k.sent_ok) || !band_ok || (int32_t)imp <= -LIM || (int32_t)imp >= LIM) {
        q.kind |= LQ_REDO;
        return;
    }
    q.lo = (int32_t)imp - (k.range + max(k.ci, 0));
    if (q.lo < -(1 << 29)) { q.kind |= LQ_REDO; return; }   // (keeps slot_vl's differences in int32)
    q.len = 0;   // empty span: no reads
    const int tid = L.chrom - 1;
    const int64_t beg = (int64_t)(uint32_t)(q.s - 1u), qend = (int64_t)(uint32_t)(q.e - 1u);
    if (tid < 0 || tid >= P.n_targets || qend <= beg) return;   // A3: no reads
    const int64_t ra = P.tid_off[tid], nr = P.tid_off[tid + 1] - ra;
    if (nr == 0) return;
    const int64_t b0 = P.bkt_off[tid], nb = P.bkt_off[tid + 1] - b0;   // last bucket = {nr, nr}
    const int64_t bh = min(qend >> BKT_SHIFT, nb - 1), bl = min(beg >> BKT_SHIFT, nb - 1);
    const uint2 h0 = P.bkt[b0 + bh], h1 = P.bkt[b0 + min(bh + 1, nb - 1)];
    const uint2 l0 = P.bkt[b0 + bl], l1 = P.bkt[b0 + min(bl + 1, nb - 1)];
    // hi = first read with pos >= qend in [h0.x, h1.x]; lo = first with emax > beg in [l0.y, l1.y]
    int64_t hl = h0.x, hh = h1.x, ll = l0.y, lh = l1.y;
    const int32_t *pp = P.pos + ra, *em = P.emax + ra;
    while (hl < hh || ll < lh) {   // the two binary searches interleaved (their loads overlap)
        const int64_t hm = (hl + hh) >> 1, lm = (ll + lh) >> 1;
        const int32_t pv = hl < hh ? pp[hm] : 0, evv = ll < lh ? em[lm] : 0;
        if (hl < hh) { if ((int64_t)pv >= qend) hh = hm; else hl = hm + 1; }
        if (ll < lh) { if ((int64_t)evv > beg) lh = lm; else ll = lm + 1; }
    }
    const int64_t lo = ra + ll, hi = ra + hl;
    if (lo >= hi) return;
    const uint64_t *off = q.kind == K_INS ? P.spoffI : P.spoffD;
    const uint64_t E0 = off[lo], E1 = off[hi];
    // spans of 2^27 events or more: the wave-wide path (lane_walk's buffer byte count)
    if (E1 - E0 >= (uint64_t)LW_BUF_MAX) { q.kind |= LQ_REDO; return; }
    q.e0[0] = (uint32_t)E0; q.e0[1] = (uint32_t)(E0 >> 32);
    q.len = (uint32_t)(E1 - E0);
}

// lane_query for the value buckets (svt_bucket.inc): A2, the window's eligibility, its band's bucket
// span and the prefix maxima's BELOW -- no region query, no binary search (one dependent step after
// the locus: the contig's bucket base, then the two bucket offsets and one prefix-max key).
__device__ __forceinline__ void lane_query_bk(const KArgs &a, uint32_t g, LvQuery &q) {
    const KParams &k = a.prm;
    const uint32_t w = g >= a.n ? 1u : 0u, li = g - w * a.n;
    const svt_locus L = a.loci[li];
    q.kind = -1;
    q.liw = li << 1 | w;
    q.len = 0;
    q.fl = 0;
    const uint32_t pos = L.pos, end = L.end;
    uint32_t imp = 0;
    if (L.type == T_INS && w == 0) { q.kind = K_INS; q.s = pos - (uint32_t)k.median; q.e = pos + (uint32_t)k.median; imp = pos; }
    else if (L.type == T_DEL && w == 0) { q.kind = K_START; q.s = pos - (uint32_t)k.wider; q.e = pos + (uint32_t)k.narrow; imp = pos; }
    else if (L.type == T_DEL) { q.kind = K_END; q.s = end - (uint32_t)k.narrow; q.e = end + (uint32_t)k.narrow; imp = end; }
    if (q.kind < 0) return;   // INV: refine_point collects only when sv_type == SV_INS (refinement.c:250): NA, NA
    BkWin W;
    const int el = bk_eligible(a, q.kind, L.chrom, q.s, q.e, imp, W);
    if (el == 0) { q.kind |= LQ_REDO; return; }   // the span-list path (refine_redo_kernel)
    q.lo = (int32_t)imp - (k.range + max(k.ci, 0));
    if (el < 0) return;                            // A3: no reads -> nb = 0 -> NA
    uint32_t E0, E1;
    bool below;
    bk_query(a.bk, q.kind, L.chrom - 1, W, E0, E1, below);
    if (E1 - E0 >= LW_BUF_MAX) { q.kind |= LQ_REDO; return; }   // (lane_walk's buffer byte count)
    q.e0[0] = E0;
    q.e0[1] = 0u;
    q.len = E1 - E0;
    q.fl = below ? LV_BELOW : 0u;
}

// LV_W windows per wave (phase 2: one lane each, so <= 64), taken through phases 0-1 LV_R at a
// time (LV_R == LV_W: one round).
template <int LV_W, bool BK>
__global__ __launch_bounds__(64 * WPB) SVT_WAVES(lane_waves(LV_W)) void refine_lane_kernel(KArgs a) {
    static_assert(LV_W <= WAVE && LV_W % LV_R == 0, "one lane per window in phase 2, whole rounds");
    __shared__ LaneLds<LV_W> lds_all[WPB];
    const uint32_t wid = threadIdx.x >> 6;
    const int ln = lane_id();
    const uint32_t g0 = (blockIdx.x * WPB + wid) * LV_W, nw = 2u * a.n;
    if (g0 >= nw) return;
    LaneLds<LV_W> &L = lds_all[wid];
    const KParams &k = a.prm;
    const uint32_t cnt = min((uint32_t)LV_W, nw - g0);
    const int32_t bw = k.range + max(k.ci, 0);   // the band's half-width
    PH(long long ph_t0 = 0, ph_t1 = 0;)
    const bool band_ok = k.range > SV_MIN_LENGTH / 2 && bw <= LV_WMAX && k.ci >= -LV_WMAX;
    // Window g0 + l is lane l's in phase 2: its row, its flags word, and (in registers) its band's
    // low end; in a round of phases 0-1 it is lane l - r0's.
    uint32_t aflags = 0;   // phase 1: the flags of a window walked alone, in its phase-2 lane
    int32_t mylo = 0;
#pragma nounroll
    for (uint32_t r0 = 0; r0 < cnt; r0 += (uint32_t)LV_R) {
    PH_T(pt0);
    // ---- phase 0: every window's A2 + A3 at once, one lane each (the dependent loads of
    // locus -> bucket words -> pos/emax searches -> span bounds run once per LV_R windows).
    // The flags word is final here unless the window has a span to walk, and the walkable
    // windows' table entries go to win[] in lane order.
    uint32_t nwin;
    {
        const bool mine = (uint32_t)ln < min((uint32_t)LV_R, cnt - r0);
        const uint32_t row = r0 + (uint32_t)ln;
        LvQuery q{};
        if (mine) {
            if (BK) lane_query_bk(a, g0 + row, q);
            else lane_query(a, g0 + row, band_ok, q);
        }
        const bool walk = mine && q.kind >= 0 && !(q.kind & LQ_REDO) && q.len != 0u;
        if (mine) {
            uint32_t *row32 = reinterpret_cast<uint32_t *>(L.stage + row * LV_S);
#pragma unroll
            for (int j = 0; j < LV_CAP / 2; j++) row32[j] = 0xffffffffu;   // unused band slots read as 0xffff
            L.flags[row] = q.kind < 0 ? LV_NONE : (q.kind & LQ_REDO) ? LV_REDO : LV_PENDING;
        }
        if constexpr (LV_R < LV_W) {   // the band's low end moves to the window's phase-2 lane
            const int32_t t = __shfl(q.lo, ln & (LV_R - 1), WAVE);
            if (((uint32_t)ln & ~(uint32_t)(LV_R - 1)) == r0) mylo = t;
        } else {
            mylo = q.lo;
        }
        const uint64_t wm = ballot(walk);
        if (walk) {
            LvWin wn;
            wn.e0 = (uint64_t)q.e0[0] | (uint64_t)q.e0[1] << 32;
            wn.s = q.s;
            wn.e = q.e;
            wn.kl = (uint32_t)q.kind | row << 8 | (q.fl ? LVW_BELOW : 0u);
            wn.len = q.len;
            L.win[mbcnt(wm)] = wn;
        }
        nwin = (uint32_t)__popcll(wm);
    }
    wave_sync();
    PH_T(pt1);
    PH(ph_t0 += pt1 - pt0;)
    // ---- phase 1 (packed): windows of <= 64 events share slots (lane_packed), longer ones are
    // walked alone (lane_walk).  Lane c holds walkable window c's walk constants, computed here
    // once for the wave; the scalar window loop reads them with v_readlane (no LDS round trip and
    // no scalar arithmetic per window), and a window walked alone leaves its flags in lane kw of
    // aflags (a v_cndmask on the lane index) instead of a store to its flags word.
    {
        const bool has = (uint32_t)ln < nwin;
        const LvWin wv = L.win[has ? (uint32_t)ln : 0u];   // (entry 0 unused when nwin == 0)
        const uint32_t lenv = has ? wv.len : 0u, klv = wv.kl & 0xffffu, ev = wv.e;
        const uint32_t flv = wv.kl & LVW_BELOW ? LV_BELOW : 0u;
        const int32_t em2v = (int32_t)(wv.e - 2u);
        const int32_t lov = lv_lo(k, klv & 0xffu, wv.s, bw);
        const int32_t b1v = max((int32_t)(wv.s - 1u), -(1 << 30)) + 1;
        const int32_t scv = (int32_t)min(wv.s, 0x7fffffffu);
        const uint64_t addrv = reinterpret_cast<uint64_t>(
            (BK ? a.bk.ev : (klv & 0xffu) == (uint32_t)K_INS ? a.pile.spI : a.pile.spD) +
            wv.e0);
        uint16_t *sink = reinterpret_cast<uint16_t *>(&L.sink[ln]);
        const int32_t bw2 = 2 * bw;
        PH({ const uint32_t tl = rdlane(wave_scan_add(lenv), WAVE - 1); if (ln == 0) { PH_ADD(8, nwin); PH_ADD(9, tl); } })
        for (uint32_t c = 0; c < nwin;) {
            const uint32_t l0 = rdlane(lenv, (int)c);
            PH(if (ln == 0) { if (l0 > (uint32_t)WAVE) { PH_ADD(10, 1); PH_ADD(11, (l0 + 255u) / 256u); } else PH_ADD(12, 1); })
            if (l0 > (uint32_t)WAVE && l0 <= 2u * WAVE && c + 1u < nwin) {   // a pair of 2-slot windows?
                const uint32_t l1 = rdlane(lenv, (int)(c + 1u));
                const uint32_t ka = rdlane(klv, (int)c), kb = rdlane(klv, (int)(c + 1u));
                if (l1 > (uint32_t)WAVE && l1 <= 2u * WAVE && ((ka ^ kb) & 0xffu) == 0u) {
                    auto one = [&](uint32_t cc, uint32_t kl, uint32_t len) {
                        const int32_t lo = rdlane_i(lov, (int)cc);
                        return LwOne{rdlane64(addrv, (int)cc), len,
                                     LwWin{rdlane_i(b1v, (int)cc), rdlane(ev, (int)cc), rdlane_i(scv, (int)cc), lo + 1,
                                           lo + bw2 - 1, (uint32_t)(bw2 - 1), rdlane_i(em2v, (int)cc)},
                                     lo, L.stage + (kl >> 8) * LV_S};
                    };
                    const LwOne A = one(c, ka, l0), B = one(c + 1u, kb, l1);
                    LaneBand ra, rb;
                    if ((ka & 0xffu) == (uint32_t)K_INS) lane_walk2<K_INS, BK>(A, B, sink, ra, rb);
                    else if ((ka & 0xffu) == (uint32_t)K_START) lane_walk2<K_START, BK>(A, B, sink, ra, rb);
                    else lane_walk2<K_END, BK>(A, B, sink, ra, rb);
                    const uint32_t fa = ra.nb > LV_CAP ? LV_REDO
                                                       : (uint32_t)ra.nb | LV_PENDING | ra.flags | rdlane(flv, (int)c);
                    const uint32_t fb = rb.nb > LV_CAP ? LV_REDO
                                                       : (uint32_t)rb.nb | LV_PENDING | rb.flags | rdlane(flv, (int)(c + 1u));
                    aflags = (uint32_t)ln == (ka >> 8) ? fa : (uint32_t)ln == (kb >> 8) ? fb : aflags;
                    c += 2u;
                    continue;
                }
            }
            if (l0 > (uint32_t)WAVE) {
                const uint32_t kl = rdlane(klv, (int)c), kind = kl & 0xffu, kw = kl >> 8;
                const int32_t lo = rdlane_i(lov, (int)c);
                const LwWin W{rdlane_i(b1v, (int)c), rdlane(ev, (int)c), rdlane_i(scv, (int)c), lo + 1, lo + bw2 - 1,
                              (uint32_t)(bw2 - 1), rdlane_i(em2v, (int)c)};
                const uint64_t base = rdlane64(addrv, (int)c);
                uint16_t *row = L.stage + kw * LV_S;
                LaneBand r;
                if (kind == (uint32_t)K_INS) r = lane_walk<K_INS, BK>(base, l0, W, lo, row, sink);
                else if (kind == (uint32_t)K_START) r = lane_walk<K_START, BK>(base, l0, W, lo, row, sink);
                else r = lane_walk<K_END, BK>(base, l0, W, lo, row, sink);
                const uint32_t f = r.nb > LV_CAP ? LV_REDO : (uint32_t)r.nb | LV_PENDING | r.flags | rdlane(flv, (int)c);
                aflags = (uint32_t)ln == kw ? f : aflags;
                c++;
                continue;
            }
            uint64_t M = 1ull;
            uint32_t tot = l0, c1 = c + 1u;
            for (; c1 < nwin; c1++) {
                const uint32_t l = rdlane(lenv, (int)c1);
                if (tot + l > (uint32_t)WAVE) break;
                M |= 1ull << tot;
                tot += l;
            }
            if (!BK) {
                lane_packed<BK>(a.pile, a.bk, k, L.win, L.flags, L.stage, c, M, tot, bw2);
                c = c1;
                continue;
            }
            // value buckets: most windows hold < 64 events, so a wave's phase 1 is a run of packed
            // slots -- each slot's events are loaded while the previous slot is tested (the loads,
            // not the tests, were the run's length: one round trip per slot, ~9 slots a wave on cfg4)
            uint4 v = lane_packed_load(a.bk, L.win, c, M);
            for (;;) {
                uint64_t Mn = 1ull;
                uint32_t totn = 0, cn1 = c1;
                const bool more = c1 < nwin && rdlane(lenv, (int)c1) <= (uint32_t)WAVE;
                if (more) {
                    totn = rdlane(lenv, (int)c1);
                    for (cn1 = c1 + 1u; cn1 < nwin; cn1++) {
                        const uint32_t l = rdlane(lenv, (int)cn1);
                        if (totn + l > (uint32_t)WAVE) break;
                        Mn |= 1ull << totn;
                        totn += l;
                    }
                }
                // (unconditional: a load under a branch would be waited for at the join)
                const uint4 vn = lane_packed_load(a.bk, L.win, more ? c1 : c, more ? Mn : M);
                lane_packed<BK>(a.pile, a.bk, k, L.win, L.flags, L.stage, c, M, tot, bw2, &v);
                c = c1;
                if (!more) break;
                v = vn;
                M = Mn;
                tot = totn;
                c1 = cn1;
            }
        }
        wave_sync();
    }
    PH(ph_t1 += wall_clock64() - pt1;)
    }   // (the round)
    PH_T(pt2);
    const bool mine = (uint32_t)ln < cnt;
    struct { int32_t lo; uint32_t liw, flags; } mt;   // the window's facts, in its own lane
    {
        const uint32_t g = g0 + (uint32_t)ln, w = g >= a.n ? 1u : 0u;
        mt.lo = mylo;
        mt.liw = (g - w * a.n) << 1 | w;
        mt.flags = mine ? L.flags[ln] : 0u;
    }
    if (aflags) mt.flags = aflags;   // the window was walked alone
    // ---- phase 2: one lane per staged window
    uint64_t redo;   // the windows left over for refine_redo_kernel
    {
        // decisions: no window or fewer than min_count band members -> NA (refinement.c:43-45,
        // LaneBand); the wave-wide path; or this lane's vote
        const bool na = mine && ((mt.flags & LV_NONE) || (!(mt.flags & LV_REDO) && (int32_t)(mt.flags & 0xffu) < k.min_count));
        if (na) write_result(a, mt.liw >> 1, mt.liw & 1u, SVT_NA);
        redo = ballot(mine && !na && (mt.flags & LV_REDO));
        const bool pend = mine && !na && !(mt.flags & LV_REDO) && (mt.flags & LV_PENDING);
        const int32_t nb = pend ? (int32_t)(mt.flags & 0xffu) : 0;
        const uint64_t any = ballot(pend);
        if (any) {
            uint32_t x[LV_CAP];
            // lanes without a staged window use row 0 read-only (rows exist for LV_W lanes only)
            uint16_t *row = L.stage + (pend ? (uint32_t)ln : 0u) * LV_S;
            const uint32_t *row32 = reinterpret_cast<const uint32_t *>(row);
#pragma unroll
            for (int j = 0; j < LV_CAP; j += 2) {   // two offsets per 4-byte LDS read
                const uint32_t v = row32[j >> 1];
                x[j] = v & 0xffffu;   // (slots past the band hold 0xffff: phase 0)
                x[j + 1] = v >> 16;
            }
            int32_t nmax = nb;   // wave max of nb: the smallest network that sorts every lane
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) nmax = max(nmax, __shfl_xor(nmax, d, WAVE));
            PH(if (ln == 0) PH_ADD(nmax <= 8 ? 13 : nmax <= 16 ? 14 : 15, 1));
            if (nmax <= 8) lv_oe_sort<0, 8>(x);
            else if (nmax <= 16) lv_oe_sort<0, 16>(x);
            else lv_oe_sort<0, 32>(x);
            uint32_t *wrow = reinterpret_cast<uint32_t *>(row);
            int32_t l0 = 0;
            if (pend) {
#pragma unroll
                for (int j = 0; j < LV_CAP; j += 2) wrow[j >> 1] = x[j] | x[j + 1] << 16;
                // the band elements <= pos + 25, counted on the sorted registers (no search)
#pragma unroll
                for (int j = 0; j < LV_CAP; j++) l0 += (int32_t)(x[j] <= (uint32_t)(bw + SV_MIN_LENGTH / 2));
                l0 = min(l0, nb);
            }
            // value buckets: ABOVE was only seen as far as the band's buckets; the vote reads it
            // only when no candidate lies below pos - 25 (lane_vote's q) -- then the wave walks for
            // it, window by window (bk_above: the bounded walks of svt_bucket.inc)
            const bool needA = BK && pend && !(mt.flags & (LV_BELOW | LV_ABOVE)) &&
                               (int32_t)x[0] >= bw - SV_MIN_LENGTH / 2;
            if (BK) {
                for (uint64_t na = ballot(needA); na; na &= na - 1ull) {
                    const int l = __builtin_ctzll(na);
                    uint32_t li, wi, ws = 0, we = 0, wimp = 0;
                    int32_t chrom;
                    const int kind = window_of(a, g0 + (uint32_t)l, li, wi, chrom, ws, we, wimp);
                    BkWin W;
                    bool ab = false;
                    if (bk_eligible(a, kind, chrom, ws, we, wimp, W) == 1) {
                        unsigned long long wk_ = 0;
                        if (kind == K_INS) ab = bk_above<K_INS>(a.bk, chrom - 1, W, wk_);
                        else if (kind == K_START) ab = bk_above<K_START>(a.bk, chrom - 1, W, wk_);
                        else ab = bk_above<K_END>(a.bk, chrom - 1, W, wk_);
                    }
                    if (ln == l && ab) mt.flags |= LV_ABOVE;
                }
            }
            if (pend) {
                const int32_t r = lane_vote(row, nb, bw, mt.lo, mt.flags, k, l0);
                write_result(a, mt.liw >> 1, mt.liw & 1u, (uint32_t)r);
            }
        }
        wave_sync();
    }
    PH_T(pt3);
    // ---- the windows voted wave-wide go to refine_redo_kernel (rare: 0.6 % of cfg4's)
    if (redo) {
        uint32_t base = 0;
        if (ln == 0) base = atomicAdd(a.redo_ctr, (uint32_t)__popcll(redo));
        base = rdlane(base, 0);
        if ((redo >> ln) & 1ull) a.redo_list[base + mbcnt(redo)] = g0 + (uint32_t)ln;
    }
    PH(if (ln == 0) { const long long pt4 = wall_clock64(); PH_ADD(0, ph_t0); PH_ADD(1, ph_t1); PH_ADD(2, pt3 - pt2); PH_ADD(3, pt4 - pt3); PH_ADD(4, 1); })
}
