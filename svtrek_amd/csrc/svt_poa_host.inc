// svt_poa_host.inc -- host half of the allele-consensus mode (included by svt_engine.hip inside its
// anonymous namespace, after svt_ctx and its helpers): the POA slot pools, poa_finish (the consensus
// launches, shared with svt_callseq_host.inc) and poa_run.  The kernels are in svt_poa.inc.

// POA scratch, kept across calls: one slot per persistent wave in two pools.  The many
// small slots hold graphs up to POA_SMALL_NODES nodes with POA_SMALL_SPILL spill rows (a
// typical allele's graph is a few thousand nodes and spills none); loci that outgrow them
// rerun on the few full-size slots.  Sizes at the default parameters: 2560 x 8.6 MB
// (10 waves per CU: the LDS ring bounds occupancy at 11) and 256 x 50 MB.
#ifndef SVT_POA_SLOTS_SMALL
#define SVT_POA_SLOTS_SMALL 2560
#endif
constexpr uint64_t POA_SLOTS_SMALL = SVT_POA_SLOTS_SMALL;
constexpr uint64_t POA_SLOTS_BIG = 256;
constexpr int32_t POA_SMALL_NODES = 16384;
constexpr int32_t POA_SMALL_SPILL = 256;

// The parameter limits of svt_poa_consensus and svt_call_consensus.
bool poa_params_ok(const svt_poa_params *p) {
    const int64_t w_max = (int64_t)p->band_b + (int64_t)p->band_f_permille * p->max_len / 1000;
    return !(p->match < 0 || p->mismatch < 0 || p->gap_open < 0 || p->gap_ext < 0 || p->band_b < 1 || p->band_f_permille < 0 ||
             p->max_seqs < 1 || p->max_seqs > POA_PIN || p->max_len < 1 || p->max_len > POA_SEQ_MAX || w_max > 63 ||
             p->max_nodes < p->max_len || p->max_nodes > 65000 || p->support_radius < 0 || p->max_support < 1 ||
             p->match > 1000 || p->mismatch > 1000 || p->gap_open > 1000 || p->gap_ext > 1000);
}

svt_status poa_pool(svt_ctx *c, PoaPool &pl, int32_t node_cap, int32_t spill_cap, const svt_poa_params *p,
                    uint64_t want) {
    const uint64_t sb = poa_slot_bytes(node_cap, spill_cap, p->max_len);
    if (pl.d && pl.slot_bytes == sb && pl.nslots >= want) return SVT_OK;
    pl.d.reset();   // (not reserve: fewer, larger slots may need fewer bytes, and get their own block)
    pl.nslots = 0;
    if (svt_status s = nomem(c, pl.d.reserve(want * sb), "poa scratch (lower max_nodes / max_len)")) return s;
    pl.slot_bytes = sb;
    pl.nslots = (uint32_t)want;
    return SVT_OK;
}

// SVTREK_POA_SMALL_NODES overrides the small slots' node budget (tests force deferral).
int32_t poa_small_cap(const svt_poa_params *p) {
    const char *ev = getenv("SVTREK_POA_SMALL_NODES");
    const int32_t want = ev ? (int32_t)atoi(ev) : POA_SMALL_NODES;
    return std::min(p->max_nodes, std::max(want, p->max_len + 2));
}

// One persistent launch of poa_kernel over d_list (or all n loci) on pool pl; synchronous.
svt_status poa_launch(svt_ctx *c, PoaArgs a, const PoaPool &pl, int32_t node_cap, int32_t spill_cap,
                      const uint32_t *d_list, uint32_t n, uint32_t *d_queue) {
    a.slots = pl.d;
    a.slot_bytes = pl.slot_bytes;
    a.node_cap = node_cap;
    a.spill_cap = spill_cap;
    a.list = d_list;
    a.n = n;
    a.queue = d_queue;
    a.diag = nullptr;
    HIP_TRY(c, hipMemset(d_queue, 0, sizeof(uint32_t)));
#if SVT_POA_DIAG
    DevBuf<unsigned long long> diag;
    HIP_TRY(c, diag.reserve(PD_N));
    a.diag = diag;
    HIP_TRY(c, hipMemset(a.diag, 0, PD_N * sizeof(unsigned long long)));
    HIP_TRY(c, hipMemset(a.diag + PD_T0, 0xff, sizeof(unsigned long long)));
#endif
    const unsigned grid = (unsigned)std::min<uint64_t>(pl.nslots, n);
    hipLaunchKernelGGL(poa_kernel, dim3(grid), dim3(64), 0, nullptr, a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipDeviceSynchronize());
#if SVT_POA_DIAG
    unsigned long long h[PD_N];
    HIP_TRY(c, hipMemcpy(h, a.diag, sizeof h, hipMemcpyDeviceToHost));
    fprintf(stderr, "poa_diag node_cap=%d grid=%u loci=%u wave-ms: support %.1f load %.1f rows %.1f trace %.1f "
            "fuse %.1f cons %.1f | rows %llu steps %llu seqs %llu far %llu\n", node_cap, grid, n, h[PD_SUPPORT] * 1e-5,
            h[PD_LOAD] * 1e-5, h[PD_ROWS] * 1e-5, h[PD_TRACE] * 1e-5, h[PD_FUSE] * 1e-5, h[PD_CONS] * 1e-5,
            h[PD_NROWS], h[PD_NSTEPS], h[PD_NSEQ], h[PD_NFAR]);
    fprintf(stderr, "poa_diag span %.1f ms, longest locus %.1f ms, busiest wave %.1f ms\n",
            (h[PD_T1] - h[PD_T0]) * 1e-5, h[PD_LOCMAX] * 1e-5, h[PD_WAVEMAX] * 1e-5);
#endif
    return SVT_OK;
}

// The consensus launches over n loci whose supports and cost estimates are in a.nsupg / a.supg / a.est
// (poa_support_kernel's, or the call gather's of svt_callseq.inc): the loci longest first (ties: input
// order) on the small slots, the deferred ones again on the full-size slots, then res and bases back to
// the host.  d_aux: [0] work queue, [1 .. n] locus order.
svt_status poa_finish(svt_ctx *c, const svt_poa_params *p, PoaArgs a, size_t n, uint32_t *d_aux, int32_t cap,
                      uint8_t *bases, svt_poa_result *res, uint64_t *n_deferred) {
    svt_status s;
    const int32_t small_cap = poa_small_cap(p);
    std::vector<uint32_t> est(n), order(n);
    HIP_TRY(c, hipMemcpy(est.data(), a.est, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return est[x] > est[y]; });
    HIP_TRY(c, hipMemcpy(d_aux + 1, order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    if ((s = poa_pool(c, c->poa_small, small_cap, POA_SMALL_SPILL, p, std::min<uint64_t>(n, POA_SLOTS_SMALL)))) return s;
    if ((s = poa_launch(c, a, c->poa_small, small_cap, POA_SMALL_SPILL, d_aux + 1, (uint32_t)n, d_aux))) return s;
    HIP_TRY(c, hipMemcpy(res, a.res, n * sizeof(int4), hipMemcpyDeviceToHost));
    std::vector<uint32_t> deferred;   // in the same longest-first order
    for (size_t q = 0; q < n; q++)
        if (res[order[q]].status == POA_DEFER) deferred.push_back(order[q]);
    *n_deferred = deferred.size();
    if (!deferred.empty()) {
        const uint32_t nd = (uint32_t)deferred.size();
        HIP_TRY(c, hipMemcpy(d_aux + 1, deferred.data(), nd * sizeof(uint32_t), hipMemcpyHostToDevice));
        if ((s = poa_pool(c, c->poa_big, p->max_nodes, p->max_nodes + 2, p, std::min<uint64_t>(nd, POA_SLOTS_BIG)))) return s;
        if ((s = poa_launch(c, a, c->poa_big, p->max_nodes, p->max_nodes + 2, d_aux + 1, nd, d_aux))) return s;
        HIP_TRY(c, hipMemcpy(res, a.res, n * sizeof(int4), hipMemcpyDeviceToHost));
    }
    if (cap > 0) HIP_TRY(c, hipMemcpy(bases, a.out, n * (size_t)cap, hipMemcpyDeviceToHost));
    return SVT_OK;
}

svt_status poa_run(svt_ctx *c, const svt_poa_params *p, const svt_locus *loci, const svt_result *refined, size_t n,
                   int32_t cap, uint8_t *bases, svt_poa_result *res) {
    DevBuf<svt_locus> d_loci;
    DevBuf<svt_result> d_ref;
    DevBuf<uint8_t> d_out;
    DevBuf<int4> d_res;
    DevBuf<uint32_t> d_aux;   // [0] work queue, [1 .. n] locus order, [n+1 .. 2n] cost estimates
    DevBuf<int32_t> d_sup;    // [n] supporting sequences found, then [n][max_support] their indices
    HIP_TRY(c, d_loci.reserve(n));
    HIP_TRY(c, d_ref.reserve(n));
    HIP_TRY(c, d_out.reserve(std::max<size_t>(1, n * (size_t)cap)));
    HIP_TRY(c, d_res.reserve(n));
    HIP_TRY(c, d_aux.reserve(2 * n + 1));
    HIP_TRY(c, d_sup.reserve(n * (1 + (size_t)p->max_support)));
    HIP_TRY(c, hipMemcpy(d_loci, loci, n * sizeof(svt_locus), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d_ref, refined, n * sizeof(svt_result), hipMemcpyHostToDevice));
    const KArgs k = make_args(c, nullptr, nullptr, 0, false);
    PoaArgs a;
    a.pile = k.pile;
    a.prm = k.prm;
    a.pp = PoaParams{p->match, p->mismatch, p->gap_open, p->gap_ext, p->band_b, p->band_f_permille,
                     p->max_seqs, p->max_len, p->max_nodes, p->support_radius, p->max_support};
    a.loci = d_loci;
    a.refined = d_ref;
    a.n = (uint32_t)n;
    a.ins_base = c->ix.d_spoffI;
    a.ins_off = c->d_ins_off;
    a.ins_bases = c->d_ins_bases;
    a.cap = cap;
    a.out = d_out;
    a.res = d_res;
    a.nsupg = d_sup;
    a.supg = d_sup + n;
    a.est = d_aux + 1 + n;
    a.diag = nullptr;
    // supports + cost estimates
    hipLaunchKernelGGL(poa_support_kernel, dim3((unsigned)std::min<size_t>(n, 8192)), dim3(64), 0, nullptr, a);
    HIP_TRY(c, hipGetLastError());
    return poa_finish(c, p, a, n, d_aux, cap, bases, res, &c->poa_deferred);
}
