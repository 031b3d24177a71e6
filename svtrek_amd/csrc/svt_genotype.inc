// svt_genotype.inc -- genotypes of DEL / INS sites from the resident index (include/svtrek_genotype.h;
// included by svt_engine.hip after svt_call.inc, the host side is svt_genotype_host.inc).
//
// One wave per site, WPB waves a workgroup; everything a wave branches on is wave-uniform, as in
// evidence_kernel and call_emit_kernel.  No CIGAR is walked and no LDS is used:
//   alt, alt_all   the items are the OP_DEL events of the value-bucket array S / the events of array I,
//                  filed by their start x, each carrying its read's extent ({x, CIGAR word, endpos, read
//                  pos}).  The buckets covering [x_lo, x_hi] are read 64 events a trip and every event
//                  is tested for its op, x (bucket ranges are whole buckets, and a contig's last bucket
//                  holds every value past the others), length and -- for alt -- its read's span.
//   span           evidence's depth with two bounds (span_reads): the region query at b, then
//                  pos <= a and endpos > b counted over its reads.
//   genotype       three 64-bit dot products and the PL arithmetic of the header, by every lane alike.
// The 32-B record is stored by lanes 0-7, one word each.  The kernel is a template on the record it
// reads: an svt_call is a site through its fields of the same names, so svt_genotype_calls runs on
// the last scan's calls where they lie.  JUNC (svt_genotype_calls after a scan with junctions = 1,
// include/svtrek_junction.h) is the instantiation for the union index: an event whose word w has
// JN_MARK set is a junction item, its extent the other 31 bits and word z; the junction items among
// alt are counted apart and do not reduce ref (the halves of a split read do not span).
static_assert(sizeof(svt_gt_site) == 32 && sizeof(svt_gt) == 32 && sizeof(svt_gt_params) == 32, "include/svtrek_genotype.h");

struct GtArgs {
    BkIndex bk;
    DevPileup pile;
    svt_gt_params prm;
    int32_t nt;      // contigs (0 for a pileup without reads: every site is invalid and no table is read)
    uint32_t n;      // sites
};

// alt_all and alt of the items of array A (op `want`) in [x_lo, x_hi] x [len_lo, len_hi]; x_hi < 2^30.
template <bool JUNC>
__device__ __forceinline__ void gt_items(const BkIndex &B, int A, uint32_t want, int tid, uint32_t x_lo, uint32_t x_hi,
                                         uint32_t len_lo, uint32_t len_hi, int64_t a, int64_t b, uint32_t &alt_all,
                                         uint32_t &alt, uint32_t &alt_j) {
    const int ln = lane_id();
    uint32_t E0, E1;
    bk_range(B, A, tid, x_lo, x_hi, E0, E1);
    for (uint32_t e0 = E0; e0 < E1; e0 += WAVE) {
        const uint32_t i = e0 + (uint32_t)ln;
        const uint4 v = i < E1 ? B.ev[i] : make_uint4(0, 0, 0, 0);
        const uint32_t len = v.y >> 4;
        const bool item = i < E1 && (v.y & 0xfu) == want && v.x >= x_lo && v.x <= x_hi && len >= len_lo && len <= len_hi;
        const uint32_t beg = JUNC ? v.w & 0x7fffffffu : v.w;
        const bool spans = (int64_t)(int32_t)beg <= a && (int64_t)(int32_t)v.z > b;   // v.w: the read's pos, v.z: its endpos
        alt_all += (uint32_t)__popcll(ballot(item));
        alt += (uint32_t)__popcll(ballot(item && spans));
        if (JUNC) alt_j += (uint32_t)__popcll(ballot(item && spans && (v.w >> 31) != 0u));
    }
}

template <typename Site, bool JUNC = false>
__global__ __launch_bounds__(64 * WPB) void genotype_kernel(GtArgs g, const Site *sites, svt_gt *out) {
    const uint32_t k = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (k >= g.n) return;
    const Site &s = sites[k];
    const int32_t type = uniform_i(s.type), chrom = uniform_i(s.chrom);
    const uint32_t pos = (uint32_t)uniform_i((int32_t)s.pos), end = (uint32_t)uniform_i((int32_t)s.end);
    const uint32_t x_lo = (uint32_t)uniform_i((int32_t)s.x_lo), x_hi = (uint32_t)uniform_i((int32_t)s.x_hi);
    const uint32_t len_lo = (uint32_t)uniform_i((int32_t)s.len_lo), len_hi = (uint32_t)uniform_i((int32_t)s.len_hi);
    bool valid = (type == SVT_DEL || type == SVT_INS) && chrom >= 1 && chrom <= g.nt && x_lo <= x_hi && len_lo <= len_hi;
    if (valid) valid = g.pile.tid_off[chrom] != g.pile.tid_off[chrom - 1];   // a contig without reads has no buckets
    uint32_t w[8] = {0u, 0u, 0u, 0u, (uint32_t)-1, 0u, 0u, 0u};
    if (valid) {
        const int tid = chrom - 1;
        const int64_t a = max((int64_t)pos - (int64_t)g.prm.flank, (int64_t)0), b = (int64_t)end + (int64_t)g.prm.flank;
        const uint32_t span = span_reads(g.pile, tid, a, b);
        const uint32_t xh = min(x_hi, IX_SAT - 1u);
        uint32_t alt_all = 0, alt = 0, alt_j = 0;
        if (x_lo <= xh) {
            if (type == SVT_INS) gt_items<JUNC>(g.bk, BA_I, OP_INS, tid, x_lo, xh, len_lo, len_hi, a, b, alt_all, alt, alt_j);
            else gt_items<JUNC>(g.bk, BA_S, OP_DEL, tid, x_lo, xh, len_lo, len_hi, a, b, alt_all, alt, alt_j);
        }
        const uint32_t alt_r = alt - alt_j;   // the ALT items of spanning pileup records
        const uint32_t ref = span > alt_r ? span - alt_r : 0u;
        w[0] = alt;
        w[1] = ref;
        w[2] = span;
        w[3] = alt_all;
        if (alt + (unsigned long long)ref != 0ull) {
            unsigned long long L[3];
#pragma unroll
            for (int q = 0; q < 3; q++)
                L[q] = (unsigned long long)ref * g.prm.ref_cost[q] + (unsigned long long)alt * g.prm.alt_cost[q];
            const int gt = L[1] < L[0] ? (L[2] < L[1] ? 2 : 1) : (L[2] < L[0] ? 2 : 0);   // ties to the lowest
            uint32_t pl[3];
#pragma unroll
            for (int q = 0; q < 3; q++) pl[q] = (uint32_t)min((L[q] - L[gt] + 500ull) / 1000ull, 65535ull);
            const uint32_t other = gt == 0 ? min(pl[1], pl[2]) : gt == 1 ? min(pl[0], pl[2]) : min(pl[0], pl[1]);
            w[4] = (uint32_t)gt;
            w[5] = min(other, 99u);
            w[6] = pl[0] | pl[1] << 16;
            w[7] = pl[2];
        }
    }
    const int ln = lane_id();
    uint32_t word = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) word = ln == i ? w[i] : word;
    if (ln < 8) reinterpret_cast<uint32_t *>(out + k)[ln] = word;
}
