// svt_callseq.inc -- the supporting sequences of discovered INS calls (include/svtrek_callseq.h;
// included by svt_engine.hip after svt_poa.inc, the host side is svt_callseq_host.inc).
//
// The value-bucket events carry no read id, so a call's sequence indices come from the pileup:
//   callseq_table_kernel   once per loaded pileup: the ITEM TABLE {x, len} of every I >= 50 op at its
//                          sequence index (spoffI[r] + the op's ordinal in read r), one lane per read --
//                          only reads that own such an op walk their CIGAR words, with the index's advance
//                          rules -- and the REACH, the largest x - read pos over the items below 2^30,
//                          by one atomicMax per wave.
//   callseq_gather_kernel  one wave per call, WPB waves a workgroup, everything branched on wave-uniform
//                          (poa_support_kernel's shape and outputs: nsupg / supg / est).  An item of the
//                          call belongs to a read with pos in [x_lo - reach, x_hi]: two partition points in
//                          the contig's sorted pos, and the reads between them own one contiguous range of
//                          the table.  The wave streams it 64 entries a trip, tests x and len, and appends
//                          the matches in k order by ballot + prefix count; it stops storing at max_support
//                          and counts on.  No atomics on the lists, no sort, no LDS.
static_assert(sizeof(svt_call) == 48, "include/svtrek_call.h");

struct CsTabArgs {
    DevPileup pile;
    uint64_t n_reads, n_ins;
    uint2 *tab;            // [n_ins] {x, len}
    uint32_t *reach;       // zeroed before the launch
};

struct CsArgs {
    DevPileup pile;
    const uint2 *tab;            // [n_ins]
    const uint64_t *ins_off;     // [n_ins + 1] (svt_load_insseq)
    const svt_call *calls;       // the window's first call
    uint32_t n;                  // calls in the window
    int32_t nt;                  // contigs
    uint32_t reach;
    int32_t max_len, max_support, max_seqs;
    int32_t *nsupg, *supg;       // PoaArgs's: [n], [n][max_support]
    uint32_t *est;               // [n]
    unsigned long long *stat;    // [0] INS calls, [1] table entries streamed, [2] the largest range
};

constexpr int CS_TAB_T = 256;

__global__ __launch_bounds__(CS_TAB_T) void callseq_table_kernel(CsTabArgs a) {
    const DevPileup &P = a.pile;
    const uint64_t r = (uint64_t)blockIdx.x * CS_TAB_T + threadIdx.x;
    int32_t far = -1;
    if (r < a.n_reads) {
        const uint64_t k0 = P.spoffI[r], k1 = min(P.spoffI[r + 1], a.n_ins);
        if (k1 > k0) {
            const uint4 rc = P.rec[r];
            const uint32_t ncig = rc.z & NCIG_MASK;
            const uint32_t *cig = P.cigar + P.off64[r];
            uint32_t cur = min(rc.x, IX_SAT);   // refinement.c:118's reference_pos
            uint64_t k = k0;
            for (uint32_t i = 0; i < ncig && k < k1; i++) {
                const uint32_t w = cig[i];
                if ((w & 0xfu) == OP_INS && (w >> 4) >= (uint32_t)SV_MIN_LENGTH) {
                    a.tab[k++] = make_uint2(cur, w >> 4);
                    if (cur < IX_SAT) far = max(far, (int32_t)(cur - rc.x));
                }
                cur = min(cur + ref_adv(w), IX_SAT);   // :141
            }
        }
    }
    const int32_t m = rdlane_i(wave_scan_max(far), WAVE - 1);
    if (lane_id() == 0 && m >= 0) atomicMax(a.reach, (uint32_t)m);
}

__global__ __launch_bounds__(64 * WPB) void callseq_gather_kernel(CsArgs g) {
    const uint32_t j = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (j >= g.n) return;
    const DevPileup &P = g.pile;
    const int ln = lane_id();
    const svt_call &c = g.calls[j];
    const int32_t type = uniform_i(c.type), chrom = uniform_i(c.chrom);
    const uint32_t x_lo = (uint32_t)uniform_i((int32_t)c.x_lo), x_hi = (uint32_t)uniform_i((int32_t)c.x_hi);
    const uint32_t len_lo = (uint32_t)uniform_i((int32_t)c.len_lo), len_hi = (uint32_t)uniform_i((int32_t)c.len_hi);
    int32_t *sup = g.supg + (uint64_t)j * (uint64_t)g.max_support;
    int nsup = -1;
    uint64_t est = 0, span = 0;
    if (type == SVT_INS) {
        nsup = 0;
        if (chrom >= 1 && chrom <= g.nt && x_lo <= x_hi) {
            const int64_t lo = P.tid_off[chrom - 1], hi = P.tid_off[chrom];
            const int64_t p_lo = max((int64_t)x_lo - (int64_t)g.reach, (int64_t)0), p_hi = (int64_t)x_hi;
            const int64_t r0 = wave_partition_point(lo, hi, [&](int64_t r) { return (int64_t)P.pos[r] >= p_lo; });
            const int64_t r1 = wave_partition_point(r0, hi, [&](int64_t r) { return (int64_t)P.pos[r] > p_hi; });
            const uint64_t k0 = P.spoffI[r0], k1 = P.spoffI[r1];   // (spoffI has n_reads + 1 entries)
            span = k1 - k0;
            const uint32_t lmax = min(len_hi, (uint32_t)g.max_len);
            for (uint64_t kb = k0; kb < k1; kb += WAVE) {
                const uint64_t k = kb + (uint64_t)ln;
                const uint2 v = k < k1 ? g.tab[k] : make_uint2(0u, 0u);
                const bool ok = k < k1 && v.x >= x_lo && v.x <= x_hi && v.x < IX_SAT && v.y >= len_lo && v.y <= lmax;
                const uint64_t m = ballot(ok);
                const int slot = nsup + (int)mbcnt(m);
                if (ok && slot < g.max_support) sup[slot] = (int32_t)k;
                nsup += __popcll(m);
            }
            poa_sync();   // the list is read back below
            const int nlist = min(nsup, g.max_support);
            int cnt = 0;
            for (int q = 0; q < nlist && cnt < g.max_seqs; q++) {   // poa_support_kernel's estimate
                const uint32_t idx = (uint32_t)uniform_i(sup[q]);
                const uint64_t m = g.ins_off[idx + 1] - g.ins_off[idx];
                if (m >= 1) { est += m; cnt++; }
            }
        }
    }
    if (ln == 0) {
        g.nsupg[j] = nsup;
        g.est[j] = (uint32_t)min(est, (uint64_t)0xffffffffu);
        if (type == SVT_INS) {
            atomicAdd(g.stat, 1ull);
            atomicAdd(g.stat + 1, (unsigned long long)span);
            atomicMax(g.stat + 2, (unsigned long long)span);
        }
    }
}
