// svt_index2.inc -- the device index of a loaded pileup, one LANE PER READ (included by
// svt_engine.hip after svt_index.inc, whose IxArgs / IxTot / totals kernel it shares).
//
// Same index as svt_index.inc's stream walk (per-read list offsets and span events -- the
// reference's per-read CIGAR walk, refinement.c:118-159 / :184-221 / :295-318, done once per
// read), different decomposition for short reads: a wave takes 64 consecutive reads (a GROUP)
// and every lane walks its own read's CIGAR serially, a 16-B vector (4 ops) at a time.  No
// marks, no cross-lane scans per op: the only cross-lane work is one wave scan per group.
// Two kernels:
//   * census: per read its D-list and I-list sizes -> cnt[r], per group the totals -> agg[g]
//     (then a hipcub exclusive scan of the groups, as in svt_index.inc); the group's ops are one
//     contiguous stretch of the stream, streamed with coalesced loads and classified per op (the
//     counts are properties of each op alone: no walk);
//   * emit: per read its list offsets (group base + wave scan of cnt), then the walk, writing its
//     span events to their slots (staged in LDS, copied out in whole rows).

#ifndef SVT_IX2_WPB
#define SVT_IX2_WPB 2
#endif
constexpr int IX2_WPB = SVT_IX2_WPB;   // waves (groups) per workgroup
#ifndef SVT_IX2_UC
#define SVT_IX2_UC 8
#endif
#ifndef SVT_IX2_UE
#define SVT_IX2_UE 8
#endif
constexpr int IX2_UC = SVT_IX2_UC;   // 16-B stream loads per lane per step: census
constexpr int IX2_UE = SVT_IX2_UE;   // ... emit

struct Ix2Args {
    IxArgs a;                 // stream, soff, rec, agg, block sums, per-read offsets, lists, caps, err
    uint2 *cnt;               // [n_reads] census -> emit: {D-list entries, I-list entries}
    uint64_t n_reads;
    uint32_t n_groups;
};

// The ops of stream[s, e) a vector at a time from the 16-B aligned s & ~3, U loads of a step
// issued together: f4(jr0, q) with jr0 the read index of q.x (wrapping for the words before s);
// words outside the read are left for f4 to mask.
template <int U, typename F>
__device__ __forceinline__ void ix2_walk4(const uint32_t *stream, uint64_t s, uint64_t e, F &&f4) {
    const uint4 *S4 = reinterpret_cast<const uint4 *>(stream);
    const uint64_t v0 = s & ~3ull;
    const uint32_t lead = (uint32_t)(s - v0), n = (uint32_t)(e - s), span = lead + n;
    for (uint32_t o = 0; o < span; o += 4 * U) {
        uint4 q[U];
#pragma unroll
        for (int u = 0; u < U; u++)
            q[u] = o + 4u * u < span ? S4[(v0 >> 2) + (o >> 2) + u] : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int u = 0; u < U; u++) f4(o + 4u * u - lead, q[u]);
    }
}

// One read's events: the walk (saturating at IX_SAT), from its list slots xD / xI on; the
// markers after its last op.
template <typename PD, typename PI>
__device__ __forceinline__ void ix2_emit_read(const IxArgs &a, uint64_t r, uint32_t xD, uint32_t xI, PD &putD, PI &putI) {
    const uint64_t s = a.soff[r], e = a.soff[r + 1];
    const uint4 rc = a.rec[r];
    const uint32_t pos = rc.x, endp = rc.y, n = (uint32_t)(e - s), clip = rc.z >> 30;
    uint32_t cur = min(pos, IX_SAT);   // refinement.c:118's reference_pos
    uint32_t dp = xD, ip = xI;         // list slots, group-relative
    // a vector at a time: the four walk positions first, then one branch for the vector's candidates
    ix2_walk4<IX2_UE>(a.stream, s, e, [&](uint32_t jr0, uint4 q) {
        uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = jr0 + (uint32_t)k < n ? w[k] : 0u;   // (a 0 word: 0M, no advance)
        uint32_t c[5];
        c[0] = cur;
#pragma unroll
        for (int k = 0; k < 4; k++) c[k + 1] = min(c[k] + ref_adv(w[k]), IX_SAT);   // refinement.c:141
        bool any = false;
#pragma unroll
        for (int k = 0; k < 4; k++) any |= ix_isDI(w[k]);
        if (any) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (ix_isD(w[k])) putD(dp++, make_uint4(c[k], w[k], endp, pos));   // :124, :188 (pos: the value
                if (ix_isI(w[k])) putI(ip++, make_uint4(c[k], w[k], endp, pos));   // :299          buckets' yield test)
            }
        }
        cur = c[4];
    });
    if (clip & SVT_CLIP_LAST_S) putD(dp++, make_uint4(cur, SP_TRAIL, endp, pos));   // :120, :147
    if (clip & SVT_CLIP_FIRST_S) putD(dp++, make_uint4(pos, SP_LEAD, endp, cur));   // :210
}

// ev: IX2_EVCAP LDS slots for the group's events -- a group whose D and I events fit is written
// to LDS during the walk and copied out in whole 16-B rows per lane afterwards (coalesced
// full-line writes instead of each lane's scattered 16-B stores); bigger groups store straight
// from the walk.
#ifndef SVT_IX2_EVCAP
#define SVT_IX2_EVCAP 320   // 5 KB a wave: 8 waves per SIMD (480: 5; index 0.644 vs 0.699 ms on cfg4, profiles/r04_v20)
#endif
constexpr uint32_t IX2_EVCAP = SVT_IX2_EVCAP;
__device__ __forceinline__ void ix2_emit(const IxArgs &a, uint64_t r, bool act, uint2 c, const IxTot &B, uint4 *ev) {
    const int ln = lane_id();
    // the lane's exclusive prefixes within the group (group totals < 2^31: host)
    uint32_t tD, tI;
    const uint32_t xD = wave_excl(c.x, tD), xI = wave_excl(c.y, tI);
    const uint64_t bD = B.v[IX_D], bI = B.v[IX_I];
    if (act) {
        a.spoffD[r] = bD + xD;
        a.spoffI[r] = bI + xI;
    }
    // the group's events go to [bD, bD + tD) and [bI, bI + tI): one wave-uniform check against
    // the census's sizes, then raw buffer descriptors of exactly that size (the hardware drops
    // anything outside)
    const bool fits = bD + tD <= a.capD && bI + tI <= a.capI;
    if (!fits && ln == 0) *a.err = 1u;
    const auto rD = __builtin_amdgcn_make_buffer_rsrc(a.spD + bD, 0, (int)uniform_i(fits ? (int)(tD * 16u) : 0), IX_RSRC);
    const auto rI = __builtin_amdgcn_make_buffer_rsrc(a.spI + bI, 0, (int)uniform_i(fits ? (int)(tI * 16u) : 0), IX_RSRC);
    const bool stage = tD + tI <= IX2_EVCAP;   // (wave-uniform)
    auto putD = [&](uint32_t i, uint4 v) {
        if (stage) ev[i] = v;
        else ix_store4(v, rD, i * 16u);
    };
    auto putI = [&](uint32_t i, uint4 v) {
        if (stage) ev[tD + i] = v;
        else ix_store4(v, rI, i * 16u);
    };
    if (act) ix2_emit_read(a, r, xD, xI, putD, putI);
    if (stage) {
        wave_sync();
        if (fits) {
            for (uint32_t i = (uint32_t)ln; i < tD; i += WAVE) a.spD[bD + i] = ev[i];
            for (uint32_t i = (uint32_t)ln; i < tI; i += WAVE) a.spI[bI + i] = ev[tD + i];
        }
        wave_sync();   // (the next group's events may reuse the slots)
    }
}

// Census, streaming.  A group's ops [soff[64g], soff[64g + 64]) are one stretch of the stream,
// so the wave reads it with coalesced 16-B loads (one load instruction covers 1 KB of
// consecutive vectors, instead of 64 lanes each in its own read's lines) and classifies every
// op; each vector's D > 50 / I >= 50 flags and their exclusive prefix counts within the step go
// to LDS (one word per vector), and every read takes its counts as the prefix at its end minus
// the prefix at its start.
constexpr int IX2_SV = WAVE * IX2_UC;   // vectors per step
static_assert(4 * IX2_SV <= 2048, "11-bit prefix fields");
struct Ix2CensusLds {
    uint32_t pv[IX2_SV];   // per vector: D prefix (11 bits) | I prefix << 11 | D flags << 22 | I flags << 26
};
__device__ __forceinline__ uint2 ix2_count_stream(const IxArgs &a, uint64_t r, bool act, uint64_t n_reads, uint32_t g,
                                                  Ix2CensusLds &L) {
    const int ln = lane_id();
    const uint64_t r1 = min((uint64_t)g * WAVE + WAVE, n_reads);
    const uint64_t s = act ? a.soff[r] : 0ull, e = act ? a.soff[r + 1] : 0ull;
    const uint32_t clip = act ? (uint32_t)a.clip8[r] : 0u;   // (1 B a read, not the 16-B record)
    const uint64_t A = rdlane64(s, 0), B = a.soff[r1];   // lane 0 always holds a read
    const uint64_t O = A & ~3ull;
    const uint32_t a0 = (uint32_t)(A - O), b1 = (uint32_t)(B - O);   // < 2^27 (host: bigger groups take the stream walk)
    const uint32_t nv = (b1 + 3u) >> 2;
    const uint32_t ps = act ? (uint32_t)(s - O) : b1, pe = act ? (uint32_t)(e - O) : b1;
    const uint4 *S4 = reinterpret_cast<const uint4 *>(a.stream + O);
    uint32_t bD = 0, bI = 0;                    // the group's counts before this step (wave-uniform)
    uint32_t sD = 0, sI = 0, eD = 0, eI = 0;    // this read's prefixes at its start / end
    bool sdone = false, edone = false;
    for (uint32_t i0 = 0; i0 < nv; i0 += (uint32_t)IX2_SV) {
        uint4 x[IX2_UC];
#pragma unroll
        for (int u = 0; u < IX2_UC; u++) {
            const uint32_t i = i0 + (uint32_t)(u * WAVE + ln);
            x[u] = i < nv ? S4[i] : make_uint4(0, 0, 0, 0);
        }
        wave_sync();   // the previous step's lookups are done with L
        uint32_t tD = 0, tI = 0;   // this step's running totals (wave-uniform)
#pragma unroll
        for (int u = 0; u < IX2_UC; u++) {
            const uint32_t ws[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
            const uint32_t j0 = 4u * (i0 + (uint32_t)(u * WAVE + ln));
            uint32_t fD = 0, fI = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t j = j0 + (uint32_t)k;
                const uint32_t w = j >= a0 && j < b1 ? ws[k] : 0u;
                fD |= ix_isD(w) ? 1u << k : 0u;
                fI |= ix_isI(w) ? 1u << k : 0u;
            }
            uint32_t tot;
            const uint32_t cnt = (uint32_t)__popc(fD) | (uint32_t)__popc(fI) << 11;
            const uint32_t ex = wave_excl(cnt, tot);
            L.pv[u * WAVE + ln] = (tD + (ex & 0x7ffu)) | (tI + (ex >> 11)) << 11 | fD << 22 | fI << 26;
            tD += tot & 0x7ffu;
            tI += tot >> 11;
        }
        wave_sync();
        const uint32_t v1 = min(i0 + (uint32_t)IX2_SV, nv);
        if (!sdone && (ps >> 2) < v1) {
            const uint32_t q = L.pv[(ps >> 2) - i0], m = (1u << (ps & 3u)) - 1u;
            sD = bD + (q & 0x7ffu) + (uint32_t)__popc((q >> 22) & m);
            sI = bI + ((q >> 11) & 0x7ffu) + (uint32_t)__popc((q >> 26) & m);
            sdone = true;
        }
        if (!edone && (pe >> 2) < v1) {
            const uint32_t q = L.pv[(pe >> 2) - i0], m = (1u << (pe & 3u)) - 1u;
            eD = bD + (q & 0x7ffu) + (uint32_t)__popc((q >> 22) & m);
            eI = bI + ((q >> 11) & 0x7ffu) + (uint32_t)__popc((q >> 26) & m);
            edone = true;
        }
        bD += tD;
        bI += tI;
    }
    if (!sdone) { sD = bD; sI = bI; }   // positions at the group's end (b1 on a vector boundary)
    if (!edone) { eD = bD; eI = bI; }
    if (!act) return make_uint2(0u, 0u);
    return make_uint2(eD - sD + ix_nmark(clip), eI - sI);
}

__global__ __launch_bounds__(64 * IX2_WPB) void ix2_census_kernel(Ix2Args A) {
    const IxArgs &a = A.a;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t g = blockIdx.x * IX2_WPB + wid;
    if (g >= A.n_groups) return;
    const uint64_t r = (uint64_t)g * WAVE + (uint64_t)lane_id();
    const bool act = r < A.n_reads;
    __shared__ Ix2CensusLds lds[IX2_WPB];
    const uint2 c = ix2_count_stream(a, r, act, A.n_reads, g, lds[wid]);
    if (act) A.cnt[r] = c;
    const uint32_t tD = rdlane(wave_scan_add(c.x), WAVE - 1), tI = rdlane(wave_scan_add(c.y), WAVE - 1);
    if (lane_id() == 0) {
        IxTot t;
        t.v[IX_D] = tD;
        t.v[IX_I] = tI;
        a.agg[g] = t;
        ix_block_add(a, g, t);
    }
}

__global__ __launch_bounds__(64 * IX2_WPB) void ix2_emit_kernel(Ix2Args A) {
    __shared__ uint4 evs[IX2_WPB][IX2_EVCAP];   // 5 KB a wave
    const IxArgs &a = A.a;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t g = blockIdx.x * IX2_WPB + wid;
    if (g >= A.n_groups) return;
    const uint64_t r = (uint64_t)g * WAVE + (uint64_t)lane_id();
    const bool act = r < A.n_reads;
    const uint2 c = act ? A.cnt[r] : make_uint2(0u, 0u);
    const IxTot B = ix_part_base(a, g);
    ix2_emit(a, r, act, c, B, &evs[wid][0]);
}
