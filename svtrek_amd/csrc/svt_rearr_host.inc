// svt_rearr_host.inc -- include/svtrek_rearr.h's entry point and the build of the rearrangement index
// (included by svt_engine.hip inside its extern "C" block after svt_junction_host.inc; svt_call_host.inc's
// scan calls rearr_build and runs its second pass over index_view(c, k.rr); the kernels are svt_rearr.inc).

extern "C++" {
namespace {

// The index of the loaded pileup's table: kept until the table changes (svt_load_junctions drops it),
// built here otherwise by callindex_build.
svt_status rearr_build(svt_ctx *c) {
    CallScratch::Rearr &r = c->call.rr;
    const CallScratch::Junction &j = c->call.jn;
    if (r.built) return SVT_OK;
    static const CallIndexText text{"svt_call_scan: the rearrangement index",
                                    "svt_call_scan: more than 2^31 - 1 rearrangement items are not supported",
                                    "rearrangement index build", 0x7fffffffull};
    RearrArgs a{};
    a.off = j.d_toff;
    a.seg = j.d_tseg;
    a.n = j.n;
    const dim3 grid((unsigned)((a.n + 64 * WPB - 1) / (64 * WPB))), block(64 * WPB);
    uint64_t tot[RR_NSTAT];
    r.stats = svt_call_rearr_stats{};
    const svt_status s = callindex_build(
        c, r, text, tot, &r.stats.build_ms,
        [&](const BkFile &f) {
            a.f = f;
            if (a.n) hipLaunchKernelGGL(rearr_kernel<true>, grid, block, 0, nullptr, a);
        },
        // (at most the table's records: svt_load_junctions bounds them by the reads)
        [](const uint64_t *t) { return CallIndexExpect{t[0] + t[1], t[0], t[0]}; },
        [&](const BkFile &f) {
            a.f = f;
            if (a.n && f.n_ev) hipLaunchKernelGGL(rearr_kernel<false>, grid, block, 0, nullptr, a);
        });
    if (s) return s;
    r.stats.dup_items = tot[0];
    r.stats.inv_items = tot[1];
    return SVT_OK;
}

}  // namespace
}  // extern "C++"

svt_status svt_call_rearr_stats_get(const svt_ctx *c, svt_call_rearr_stats *out) {
    if (!c || !out) return SVT_EINVAL;
    *out = c->call.last.rearr_stats;
    return SVT_OK;
}
