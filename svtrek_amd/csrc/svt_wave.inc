// svt_wave.inc -- wave64 primitives shared by every kernel of the engine (included first by
// svt_engine.hip): ballots and readlanes, the wave-scope sync, DPP scans, lane_xor, ref_adv, mbcnt,
// and the SVT_PHASE_PROF hooks PH() / PH_T() / PH_ADD().

// ------------------------------------------------------------------ wave primitives
#define SVT_COLD __forceinline__   // (cold paths inlined: out-of-line calls measured slower)
__device__ __forceinline__ int lane_id() { return (int)__lane_id(); }
// The lane mask of p straight from its compare (no v_cndmask / v_cmp round trip through a VGPR).
__device__ __forceinline__ uint64_t ballot(bool p) { return (uint64_t)__builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ uint32_t rdlane(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ int32_t rdlane_i(int32_t v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ uint64_t rdlane64(uint64_t v, int l) {
    uint32_t lo = rdlane((uint32_t)v, l), hi = rdlane((uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ int32_t uniform_i(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }
// Every window is owned by ONE wave (several independent waves share a workgroup), so the
// only ordering ever needed is between the lanes of a wave: a workgroup-scope
// release/acquire pair around a wave barrier (no s_barrier across the workgroup).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int CTRL, int ROWMASK>
__device__ __forceinline__ uint32_t dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWMASK, 0xf, false);
}
template <int CTRL, int ROWMASK>
__device__ __forceinline__ int32_t dpp_i(int32_t v, int32_t identity) {
    return __builtin_amdgcn_update_dpp(identity, v, CTRL, ROWMASK, 0xf, false);
}
// DPP controls (GFX9): row_shr:n = 0x110+n, wave_shr:1 = 0x138, row_bcast:15 = 0x142, row_bcast:31 = 0x143

// Inclusive wave64 prefix sum (mod 2^32).
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v) {
    v += dpp<0x111, 0xf>(v);
    v += dpp<0x112, 0xf>(v);
    v += dpp<0x114, 0xf>(v);
    v += dpp<0x118, 0xf>(v);
    v += dpp<0x142, 0xa>(v);
    v += dpp<0x143, 0xc>(v);
    return v;
}

// Inclusive wave64 max scan (identity -1).
__device__ __forceinline__ int32_t wave_scan_max(int32_t v) {
    v = max(v, dpp_i<0x111, 0xf>(v, -1));
    v = max(v, dpp_i<0x112, 0xf>(v, -1));
    v = max(v, dpp_i<0x114, 0xf>(v, -1));
    v = max(v, dpp_i<0x118, 0xf>(v, -1));
    v = max(v, dpp_i<0x142, 0xa>(v, -1));
    v = max(v, dpp_i<0x143, 0xc>(v, -1));
    return v;
}

__device__ __forceinline__ int64_t wave_scan_add64(int64_t x) {
    int l = lane_id();
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        int64_t y = __shfl_up(x, (unsigned)d, WAVE);
        if (l >= d) x += y;
    }
    return x;
}

// First index in [l, h) whose key satisfies pred (pred monotone false..true), 64-ary.
template <typename Pred>
__device__ SVT_COLD int64_t wave_partition_point(int64_t l, int64_t h, Pred pred) {   // cold: > 64 reads per bucket
    const int ln = lane_id();
    while (h - l > WAVE) {
        int64_t span = h - l;
        int64_t p = l + ((int64_t)(ln + 1) * span) / (WAVE + 1);
        uint64_t m = ballot(pred(p));
        int k = m ? __builtin_ctzll(m) : WAVE;
        int64_t nl = k == 0 ? l : l + ((int64_t)k * span) / (WAVE + 1) + 1;
        int64_t nh = k == WAVE ? h : l + ((int64_t)(k + 1) * span) / (WAVE + 1) + 1;
        l = nl;
        h = nh < h ? nh : h;
    }
    int64_t p = l + ln;
    uint64_t m = ballot(p < h && pred(p));
    return m ? l + __builtin_ctzll(m) : h;
}

// ------------------------------------------------------------------ shared helpers
__device__ __forceinline__ uint32_t ref_adv(uint32_t w) {   // refinement.c:141: every op but I (1) and S (4)
    return (w >> 4) & (uint32_t)__builtin_amdgcn_sbfe((int)~0x12u, w & 0xfu, 1);
}

__device__ __forceinline__ uint32_t mbcnt(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// x of lane ln ^ J without an LDS round trip: DPP quad permutes (1, 2), row shifts (4), row
// rotate (8), and gfx950's permlane swaps (16, 32).  A swap of x with itself yields the two
// halves {[lo, lo], [hi, hi]} (rows for 16); whichever of them does not hold this lane's own
// value at this lane holds the partner's (and if both do, the two values are equal).
template <int J>
__device__ __forceinline__ int32_t lane_xor(int32_t x) {
    if constexpr (J == 1) {
        return __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
    } else if constexpr (J == 2) {
        return __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xf, 0xf, false);   // quad_perm [2,3,0,1]
    } else if constexpr (J == 4) {
        const int32_t up = __builtin_amdgcn_update_dpp(0, x, 0x104, 0xf, 0xf, false);   // row_shl:4 (lane + 4)
        const int32_t dn = __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);   // row_shr:4 (lane - 4)
        return (lane_id() & 4) ? dn : up;
    } else if constexpr (J == 8) {
        return __builtin_amdgcn_update_dpp(0, x, 0x128, 0xf, 0xf, false);   // row_ror:8
    } else if constexpr (J == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap((uint32_t)x, (uint32_t)x, false, false);
        return (int32_t)((int32_t)r[0] == x ? r[1] : r[0]);
    } else {
        static_assert(J == 32, "lane_xor: J in {1, 2, 4, 8, 16, 32}");
        const auto r = __builtin_amdgcn_permlane32_swap((uint32_t)x, (uint32_t)x, false, false);
        return (int32_t)((int32_t)r[0] == x ? r[1] : r[0]);
    }
}
__device__ __forceinline__ int32_t lane_xor(int32_t x, int j) {   // j a compile-time constant after unrolling
    switch (j) {
        case 1: return lane_xor<1>(x);
        case 2: return lane_xor<2>(x);
        case 4: return lane_xor<4>(x);
        case 8: return lane_xor<8>(x);
        case 16: return lane_xor<16>(x);
        default: return lane_xor<32>(x);
    }
}

// SVT_PHASE_PROF (diagnostic builds): every wave of refine_lane_kernel adds its phases' wall
// time (100 MHz ticks) and work counts into ph_prof, read (and cleared) by svt_diag_phase.
#ifndef SVT_PHASE_PROF
#define SVT_PHASE_PROF 0
#endif
// PH(...) / PH_T(t): the instrumentation's statements, compiled out of the product.
#if SVT_PHASE_PROF
__device__ unsigned long long ph_prof[16];
#define PH_ADD(i, v) atomicAdd(&ph_prof[i], (unsigned long long)(v))
#define PH(...) __VA_ARGS__
#define PH_T(t) const long long t = wall_clock64()
#else
#define PH(...)
#define PH_T(t)
#endif
