// svt_callindex.inc -- what the builds of svt_call_scan's derived indexes share on the device (included
// by svt_engine.hip before svt_callmerge.inc, svt_junction.inc and svt_rearr.inc; the host side is
// svt_callindex_host.inc).  The segment table's junctions -- jn_next, jn_classify -- live in svt_jnclass.h,
// free of HIP and tested on the CPU; their limits are set at the end of this file.
//
// Each of those indexes has the value buckets' shape -- 16-B events filed by x under the main index's
// cbase / cnb / nbk, an off[BA_N][nbk + 1] table of which rows S and I are filled -- and is built by two
// passes of one kernel: COUNT adds every item to its (row, bucket)'s count, an exclusive sum per row
// turns the counts into extents, the second pass files every item through its bucket's atomic cursor.
// The order inside a bucket is whatever the atomics give.  No LDS, no inline assembly.
constexpr uint32_t BK_SLOTS = 1024;   // a build's stats are added into BK_SLOTS x N counters by wave number
                                      // (same-address atomics from every wave serialise in the L2)

// The fields every build kernel's arguments share (filled by callindex_build).
struct BkFile {
    const uint64_t *cbase;        // the main index's
    const uint32_t *cnb;
    uint64_t nbk;
    uint32_t *off;                // [BA_N][nbk + 1]: COUNT the counts of rows S and I, else their extents
    uint32_t *cur;                // [2][nbk + 1] cursors of the filing pass (zeroed)
    uint4 *ev;
    uint32_t n_ev;
    unsigned long long *stat;     // [BK_SLOTS][N] (COUNT)
    uint32_t *err;                // set when a slot falls outside its bucket's extent
};

// One item of row T (false: S, true: I) in bucket g: counted, or filed behind the bucket's first `skip`
// events (the union's base events; 0 elsewhere).  The check is the strictest the three builds had; on a
// consistent count none of its terms fires.  (T is a bool and svt_jnclass.h's jn_next walks a pointer because the other
// spellings cost rearr_kernel and junction_kernel up to three VGPRs: profiles/call_index/README.md.)
template <bool COUNT>
__device__ __forceinline__ void bk_file(const BkFile &f, bool T, uint64_t g, uint32_t skip, const uint4 &e) {
    const uint64_t row = (uint64_t)(T ? BA_I : BA_S) * (f.nbk + 1);
    if (COUNT) {
        atomicAdd(&f.off[row + g], 1u);
    } else {
        const uint32_t o0 = f.off[row + g] + skip, o1 = f.off[row + g + 1];
        const uint32_t sl = atomicAdd(&f.cur[(uint64_t)T * (f.nbk + 1) + g], 1u);
        if (o0 > o1 || sl >= o1 - o0 || o0 + sl >= f.n_ev) *f.err = 1u;
        else f.ev[o0 + sl] = e;
    }
}

// A wave's N counters summed over its lanes and added, where not zero, into the slot of the wave's
// number in a grid of 64 * WPB threads a block.
template <int N>
__device__ __forceinline__ void bk_stat_add(const BkFile &f, uint32_t (&v)[N]) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
#pragma unroll
        for (int q = 0; q < N; q++) v[q] += (uint32_t)__shfl_xor((int)v[q], d, WAVE);
    if (lane_id() == 0) {
        const uint64_t wv = (uint64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
        unsigned long long *q = f.stat + (uint64_t)N * (uint32_t)(wv & (BK_SLOTS - 1u));
#pragma unroll
        for (int j = 0; j < N; j++)
            if (v[j]) atomicAdd(&q[j], (unsigned long long)v[j]);
    }
}

// What jn_classify (svt_jnclass.h) is given: the engine's thresholds and clamps.  A junction event is
// {x, len << 4 | op, extent end, extent begin | JN_MARK}: bit 31 of the word in which a CIGAR event keeps its
// read's pos (< 2^31) marks it, so both extent words stop at JN_EXT_MAX.
constexpr uint32_t JN_MARK = 0x80000000u, JN_EXT_MAX = 0x7fffffffu;
constexpr uint32_t CM_LEN_MAX = (1u << 28) - 1u;   // an event's len field
__device__ __forceinline__ JnLimits jn_limits() { return JnLimits{SV_MIN_LENGTH, IX_SAT, CM_LEN_MAX, JN_EXT_MAX}; }
