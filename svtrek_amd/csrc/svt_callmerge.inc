// svt_callmerge.inc -- a read's fragmented D / I ops joined into merged items (include/svtrek_call.h,
// svt_call_params.merge_gap > 0; included by svt_engine.hip after svt_callindex.inc, whose BkFile,
// bk_file and bk_stat_add it uses; the host side is svt_callmerge_host.inc).
//
// The merged items go into a SECOND index with the value buckets' own shape -- 16-B events {x,
// L << 4 | OP_DEL / OP_INS, endpos, read pos} filed by x under the main index's cbase / cnb / nbk, an
// off[BA_N][nbk + 1] table of which rows S and I are filled -- so that call_sort_kernel ..
// call_emit_kernel, the split kernels and genotype_kernel run on it unchanged.  It is built by the two
// passes of svt_callindex.inc, both of them callmerge_kernel's walk over the CIGAR stream.
//
// The walk, a TEAM of lanes per read and TEAM ops a trip -- the whole wave for long reads (coalesced
// 256-B loads of the stream), 16 lanes and four reads a wave for short ones (callmerge_build picks by
// the pileup's mean read length, as the index build does); in the words of a 64-lane team:
//   x          a 64-bit inclusive prefix sum of the ops' advances across the lanes (wave_scan_add64)
//              on top of the carry of the trips before: unsaturated, as the header defines it.
//   fragments  per type T a ballot of the lanes whose op is a D / I of len >= merge_min.  A fragment
//              lane takes the PREVIOUS fragment's tail from the highest set bit of that ballot below
//              itself (one 64-bit shuffle), the first one of a trip from the open run carried in;
//              x - tail > merge_gap (or no previous fragment) makes it a HEAD.
//   runs       a second ballot holds the heads.  A fragment's run starts at the highest head at or
//              below its lane, or -- none -- is the open run; the run's sum of len up to the lane is a
//              difference of one more 64-bit prefix sum (plus the open run's sum).  The lane whose next
//              fragment in the trip is a head CLOSES its run and emits it; an open run closes when the
//              trip's first fragment is a head, and at the read's end.  The trip's last fragment leaves
//              the open run {first x, sum, tail, fragments} to the next trip, taken by readlane.
// Both types go through the same code in the same pass; a trip without a fragment of a type costs
// that type one ballot.  No LDS, no serial loop over lanes; the loops and the per-type skip are
// wave-uniform, the rest is predicated per lane.
constexpr int CM_NSTAT = 4;           // fragments, runs, joined items, items

struct CallMergeArgs {
    const uint32_t *stream;       // the CIGAR stream
    const uint64_t *soff;         // [n_reads + 1]
    const uint4 *rec;             // {pos, endpos, n_cigar | clip << 30, contig}
    uint64_t n_reads;
    BkFile f;                     // stat: [BK_SLOTS][CM_NSTAT]
    uint32_t gap, min_len;
};

// One closed run of type T (0 DEL, 1 INS): counted or filed when it is an item.  Returns whether it is.
template <bool COUNT>
__device__ __forceinline__ bool cm_emit(const CallMergeArgs &a, int T, uint64_t fx, uint64_t L, uint64_t cb, uint32_t nbt,
                                        uint32_t pos, uint32_t endp) {
    if (!(T ? L >= (uint64_t)SV_MIN_LENGTH : L > (uint64_t)SV_MIN_LENGTH)) return false;
    const uint32_t x = (uint32_t)min(fx, (uint64_t)IX_SAT), len = (uint32_t)min(L, (uint64_t)CM_LEN_MAX);
    bk_file<COUNT>(a.f, T, cb + min(x >> BKS, nbt - 1u), 0u, make_uint4(x, len << 4 | (T ? OP_INS : OP_DEL), endp, pos));
    return true;
}

__device__ __forceinline__ uint64_t cm_shfl64(uint64_t v, int l) { return (uint64_t)__shfl((long long)v, l, WAVE); }

// Inclusive 64-bit prefix sum over each team of TEAM consecutive lanes (TEAM == WAVE: wave_scan_add64).
template <int TEAM>
__device__ __forceinline__ uint64_t cm_scan64(uint64_t v, int tl) {
    if (TEAM == WAVE) return (uint64_t)wave_scan_add64((int64_t)v);
#pragma unroll
    for (int d = 1; d < TEAM; d <<= 1) {
        const uint64_t y = (uint64_t)__shfl_up((long long)v, (unsigned)d, TEAM);
        if (tl >= d) v += y;
    }
    return v;
}

// What a 64-lane team holds once per read stays wave-uniform (scalar registers): cm_uni / cm_pick are
// readlanes for TEAM == WAVE and leave the per-lane value / the shuffle to the 16-lane teams.
template <int TEAM>
__device__ __forceinline__ uint64_t cm_uni64(uint64_t v) { return TEAM == WAVE ? rdlane64(v, 0) : v; }
template <int TEAM>
__device__ __forceinline__ uint32_t cm_uni(uint32_t v) { return TEAM == WAVE ? rdlane(v, 0) : v; }
template <int TEAM>
__device__ __forceinline__ uint64_t cm_pick64(uint64_t v, int l) { return TEAM == WAVE ? rdlane64(v, l) : cm_shfl64(v, l); }

// TEAM lanes walk one read, TEAM ops a trip: the whole wave (long reads) or 16 lanes, four reads a
// wave (short reads: a 30-op read would leave 3/4 of a wave's trip idle and the build is bound by
// the waves' dependent loads, not by their arithmetic).  The ballots are the wave's, cut to the
// team's lanes; what was wave-uniform state is per lane, equal across a team.
template <bool COUNT, int TEAM>
__global__ __launch_bounds__(64 * WPB) void callmerge_kernel(CallMergeArgs a) {
    constexpr int RPW = WAVE / TEAM;   // reads per wave
    const uint64_t wv = (uint64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
    if (wv * RPW >= a.n_reads) return;
    const int ln = lane_id(), tl = ln & (TEAM - 1), tb = ln & ~(TEAM - 1);   // lane in the team, the team's first lane
    const uint64_t r = wv * RPW + (uint64_t)(ln / TEAM);
    const bool act = r < a.n_reads;
    const uint4 rc = act ? a.rec[r] : make_uint4(0, 0, 0, 0);
    const uint32_t pos = cm_uni<TEAM>(rc.x), endp = cm_uni<TEAM>(rc.y), tid = cm_uni<TEAM>(rc.w);
    const uint64_t s = cm_uni64<TEAM>(act ? a.soff[r] : 0ull), e = cm_uni64<TEAM>(act ? a.soff[r + 1] : 0ull);
    const uint64_t cb = act ? a.f.cbase[tid] : 0ull;
    const uint32_t nbt = act ? a.f.cnb[tid] : 1u;
    const uint64_t tmask = TEAM == WAVE ? ~0ull : ((1ull << (TEAM & 63)) - 1ull) << tb;
    const uint64_t below = ((1ull << ln) - 1ull) & tmask, upto = ((2ull << ln) - 1ull) & tmask;   // (lane 63: 2 << 63 == 0, all ones)
    uint64_t carry = pos;                       // the walk position before the trip's first op
    bool open[2] = {false, false};              // per type the run left open by the trips before
    uint64_t ofx[2] = {0, 0}, osum[2] = {0, 0}, otail[2] = {0, 0};
    uint32_t onf[2] = {0, 0};                   //   its fragments
    uint32_t st_frag = 0, st_runs = 0, st_join = 0, st_items = 0;   // (frag, runs: the team's, in every lane of it)
    for (uint64_t base = s; ballot(base < e); base += TEAM) {
        const uint64_t i = base + (uint64_t)tl;
        const uint32_t w = i < e ? a.stream[i] : 0u;   // (a 0 word: 0M, no advance, no fragment; a team past its read idles)
        const uint32_t op = w & 0xfu, len = w >> 4, adv = ref_adv(w);
        const uint64_t incl = cm_scan64<TEAM>(adv, tl);
        const uint64_t x = carry + incl - adv;
        carry += cm_pick64<TEAM>(incl, tb + TEAM - 1);
#pragma unroll
        for (int T = 0; T < 2; T++) {
            const bool f = op == (T ? OP_INS : OP_DEL) && len >= a.min_len;
            const uint64_t wmask = ballot(f);
            if (wmask == 0ull) continue;
            const uint64_t mask = wmask & tmask;      // the team's fragments (none: the team only takes part in the shuffles)
            const bool any = mask != 0ull;
            const uint64_t mytail = T ? x : x + len;
            // the previous fragment of the type: in the trip, or the open run's last
            const uint64_t bm = mask & below;
            const uint64_t ptl = cm_shfl64(mytail, bm ? 63 - __builtin_clzll(bm) : ln);
            const uint64_t ptail = bm ? ptl : otail[T];
            const bool hasprev = bm != 0ull || open[T];
            const bool head = f && !(hasprev && x - ptail <= (uint64_t)a.gap);
            const uint64_t hmask = ballot(head) & tmask;
            // the run of a fragment lane: from the highest head at or below it, else the open run
            const uint64_t cs = cm_scan64<TEAM>(f ? len : 0u, tl);
            const uint64_t hb = hmask & upto;
            const int h = hb ? 63 - __builtin_clzll(hb) : ln;
            const uint64_t hx = cm_shfl64(x, h), hcs = cm_shfl64(cs - (f ? len : 0u), h);
            const uint64_t fx = hb ? hx : ofx[T];
            const uint64_t L = hb ? cs - hcs : osum[T] + cs;
            const uint32_t nf = (uint32_t)__popcll(mask & upto & ~(hb ? (1ull << h) - 1ull : 0ull)) + (hb ? 0u : onf[T]);
            // the open run closes when the trip's first fragment is a head (that lane emits it)
            const int first = any ? __builtin_ctzll(mask) : ln;
            if (any && open[T] && ln == first && ((hmask >> first) & 1ull)) {
                const bool it = cm_emit<COUNT>(a, T, ofx[T], osum[T], cb, nbt, pos, endp);
                st_items += it ? 1u : 0u;
                st_join += it && onf[T] >= 2u ? 1u : 0u;
            }
            // a lane whose next fragment in the trip is a head closes its run
            const uint64_t am = mask & ~upto;
            const bool closes = f && am != 0ull && ((hmask >> __builtin_ctzll(am ? am : 1ull)) & 1ull);
            if (closes) {
                const bool it = cm_emit<COUNT>(a, T, fx, L, cb, nbt, pos, endp);
                st_items += it ? 1u : 0u;
                st_join += it && nf >= 2u ? 1u : 0u;
            }
            // the trip's last fragment leaves the open run
            const int last = any ? 63 - __builtin_clzll(mask) : ln;
            const uint64_t nfx = cm_pick64<TEAM>(fx, last), nsum = cm_pick64<TEAM>(L, last), ntail = cm_pick64<TEAM>(mytail, last);
            const uint32_t nnf = TEAM == WAVE ? rdlane(nf, last) : (uint32_t)__shfl((int)nf, last, WAVE);
            if (any) {
                ofx[T] = nfx;
                osum[T] = nsum;
                otail[T] = ntail;
                onf[T] = nnf;
                open[T] = true;
                st_frag += (uint32_t)__popcll(mask);
                st_runs += (uint32_t)__popcll(hmask);
            }
        }
    }
#pragma unroll
    for (int T = 0; T < 2; T++) {   // the runs still open at the read's end
        if (open[T] && tl == 0) {
            const bool it = cm_emit<COUNT>(a, T, ofx[T], osum[T], cb, nbt, pos, endp);
            st_items += it ? 1u : 0u;
            st_join += it && onf[T] >= 2u ? 1u : 0u;
        }
    }
    if (COUNT && ballot(st_frag != 0u)) {
        uint32_t v[CM_NSTAT] = {tl == 0 ? st_frag : 0u, tl == 0 ? st_runs : 0u, st_join, st_items};
        bk_stat_add(a.f, v);
    }
}
