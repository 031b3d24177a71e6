// svt_callseq_host.inc -- include/svtrek_callseq.h's entry points (included by svt_engine.hip inside its
// extern "C" block after svt_genotype_host.inc; the kernels are svt_callseq.inc, the consensus launches
// poa_finish of svt_poa_host.inc).

extern "C++" {
namespace {

constexpr const char *CS_MEM = "svt_call_consensus: device scratch";

// The item table and the reach of the loaded pileup: built by the first svt_call_consensus.
svt_status callseq_prepare(svt_ctx *c) {
    CallSeqScratch &k = c->callseq;
    if (k.ready) return SVT_OK;
    svt_status s;
    if ((s = nomem(c, k.d_ctr.reserve(4), CS_MEM)) || (s = nomem(c, k.d_tab.reserve(std::max<uint64_t>(c->n_ins, 1)), CS_MEM)))
        return s;
    DevEvent e0, e1;
    HIP_TRY(c, e0.create());
    HIP_TRY(c, e1.create());
    HIP_TRY(c, hipMemsetAsync(k.d_ctr, 0, 4 * sizeof(unsigned long long), nullptr));
    HIP_TRY(c, hipEventRecord(e0, nullptr));
    if (c->n_ins && c->n_reads) {
        CsTabArgs t{};
        t.pile = pile_view(c);
        t.n_reads = (uint64_t)c->n_reads;
        t.n_ins = c->n_ins;
        t.tab = k.d_tab;
        t.reach = reinterpret_cast<uint32_t *>(k.d_ctr.get());
        hipLaunchKernelGGL(callseq_table_kernel, dim3((unsigned)((t.n_reads + CS_TAB_T - 1) / CS_TAB_T)), dim3(CS_TAB_T), 0,
                           nullptr, t);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipEventRecord(e1, nullptr));
    HIP_TRY(c, hipEventSynchronize(e1));
    HIP_TRY(c, hipMemcpy(&k.reach, k.d_ctr, sizeof(uint32_t), hipMemcpyDeviceToHost));
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, e0, e1));
    k.stats = svt_call_consensus_stats{};
    k.stats.items = c->n_ins;
    k.stats.reach = k.reach;
    k.stats.table_ms = ms;
    k.ready = true;
    return SVT_OK;
}

svt_status callseq_run(svt_ctx *c, const svt_poa_params *p, uint64_t first, size_t n, int32_t cap, uint8_t *bases,
                       svt_poa_result *res) {
    CallSeqScratch &k = c->callseq;
    svt_status s = order_on(c, nullptr);   // after every launch already issued
    if (s) return s;
    if ((s = callseq_prepare(c))) return s;
    DevBuf<uint8_t> d_out;
    DevBuf<int4> d_res;
    DevBuf<uint32_t> d_aux;   // [0] work queue, [1 .. n] call order, [n+1 .. 2n] cost estimates
    DevBuf<int32_t> d_sup;    // [n] supporting sequences found, then [n][max_support] their indices
    if ((s = nomem(c, d_out.reserve(std::max<size_t>(1, n * (size_t)cap)), CS_MEM)) || (s = nomem(c, d_res.reserve(n), CS_MEM)) ||
        (s = nomem(c, d_aux.reserve(2 * n + 1), CS_MEM)) || (s = nomem(c, d_sup.reserve(n * (1 + (size_t)p->max_support)), CS_MEM)))
        return s;
    DevEvent e0, e1, e2;
    HIP_TRY(c, e0.create());
    HIP_TRY(c, e1.create());
    HIP_TRY(c, e2.create());
    const KArgs ka = make_args(c, nullptr, nullptr, 0, false);
    CsArgs g{};
    g.pile = ka.pile;
    g.tab = k.d_tab;
    g.ins_off = c->d_ins_off;
    g.calls = c->call.d_calls + first;
    g.n = (uint32_t)n;
    g.nt = c->n_reads ? c->n_targets : 0;
    g.reach = k.reach;
    g.max_len = p->max_len;
    g.max_support = p->max_support;
    g.max_seqs = p->max_seqs;
    g.nsupg = d_sup;
    g.supg = d_sup + n;
    g.est = d_aux + 1 + n;
    g.stat = k.d_ctr + 1;
    HIP_TRY(c, hipMemsetAsync(k.d_ctr + 1, 0, 3 * sizeof(unsigned long long), nullptr));
    HIP_TRY(c, hipEventRecord(e0, nullptr));
    hipLaunchKernelGGL(callseq_gather_kernel, dim3((unsigned)((n + WPB - 1) / WPB)), dim3(64 * WPB), 0, nullptr, g);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(e1, nullptr));
    PoaArgs a{};
    a.pile = ka.pile;
    a.prm = ka.prm;
    a.pp = PoaParams{p->match, p->mismatch, p->gap_open, p->gap_ext, p->band_b, p->band_f_permille,
                     p->max_seqs, p->max_len, p->max_nodes, p->support_radius, p->max_support};
    a.n = (uint32_t)n;
    a.ins_base = c->ix.d_spoffI;
    a.ins_off = c->d_ins_off;
    a.ins_bases = c->d_ins_bases;
    a.cap = cap;
    a.out = d_out;
    a.res = d_res;
    a.nsupg = g.nsupg;
    a.supg = g.supg;
    a.est = g.est;
    uint64_t deferred = 0;
    if ((s = poa_finish(c, p, a, n, d_aux, cap, bases, res, &deferred))) return s;
    HIP_TRY(c, hipEventRecord(e2, nullptr));
    HIP_TRY(c, hipEventSynchronize(e2));
    unsigned long long st[3] = {};
    HIP_TRY(c, hipMemcpy(st, k.d_ctr + 1, sizeof st, hipMemcpyDeviceToHost));
    float gms = 0.f, pms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&gms, e0, e1));
    HIP_TRY(c, hipEventElapsedTime(&pms, e1, e2));
    k.stats.ins_calls = st[0];
    k.stats.window_items = st[1];
    k.stats.window_max = st[2];
    k.stats.deferred = deferred;
    k.stats.gather_ms = gms;
    k.stats.poa_ms = pms;
    return SVT_OK;
}

}  // namespace
}  // extern "C++"

svt_status svt_call_consensus(svt_ctx *c, const svt_poa_params *p, uint64_t first, uint64_t n, int32_t cap, uint8_t *bases,
                              svt_poa_result *res) {
    if (!c || !p) return SVT_EINVAL;
    if (!c->loaded) return fail(c, SVT_ESTATE, "%s", "svt_load_pileup not called");
    if (!c->call.scanned) return fail(c, SVT_ESTATE, "%s", "svt_call_consensus: no svt_call_scan of the loaded pileup");
    if (c->call.last.merged)
        return fail(c, SVT_ESTATE, "%s", "svt_call_consensus: the last scan merged fragments (merge_gap > 0): no inserted bases for merged calls");
    if (c->call.last.junction)
        return fail(c, SVT_ESTATE, "%s", "svt_call_consensus: the last scan read split alignments (junctions = 1): no inserted bases for junction calls");
    if (!c->insseq_loaded) return fail(c, SVT_ESTATE, "%s", "svt_load_insseq not called");
    if (c->call.last.rearr)
        return fail(c, SVT_ESTATE, "%s", "svt_call_consensus: the last scan called rearrangements (rearr != 0): scan without them for inserted bases");
    if (c->call.last.bnd)
        return fail(c, SVT_ESTATE, "%s", "svt_call_consensus: the last scan called breakends (bnd = 1): scan without them for inserted bases");
    if (first > c->call.n_calls || n > c->call.n_calls - first)
        return fail(c, SVT_EINVAL, "%s", "svt_call_consensus: range past the scanned calls");
    if (n == 0) return SVT_OK;
    if (!res || cap < 0 || (cap > 0 && !bases)) return fail(c, SVT_EINVAL, "%s", "null arrays / cap");
    if (n > 0x3fffffffull) return fail(c, SVT_EINVAL, "%s", "batch too large");
    if (!poa_params_ok(p)) return fail(c, SVT_EINVAL, "%s", "poa params out of range");
    DEV_GUARD(c);
    return callseq_run(c, p, first, (size_t)n, cap, bases, res);
}

svt_status svt_call_consensus_stats_get(const svt_ctx *c, svt_call_consensus_stats *out) {
    if (!c || !out) return SVT_EINVAL;
    *out = c->callseq.stats;
    return SVT_OK;
}
