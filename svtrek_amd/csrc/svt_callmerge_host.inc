// svt_callmerge_host.inc -- the build of the merged index (included by svt_engine.hip inside its
// extern "C" block after svt_callindex_host.inc and before svt_call_host.inc, whose scan calls it; the
// kernel is svt_callmerge.inc).

extern "C++" {
namespace {

// The merged index of the loaded pileup for (gap, min_len): kept until either changes, built here
// otherwise by callindex_build with callmerge_kernel's walk as both passes.
svt_status callmerge_build(svt_ctx *c, uint32_t gap, uint32_t min_len) {
    CallScratch::Merged &m = c->call.mg;
    if (m.built && m.gap == gap && m.min_len == min_len) return SVT_OK;
    static const CallIndexText text{"svt_call_scan: the merged index", "svt_call_scan: 2^31 merged events and more are not supported",
                                    "merged index build", 0x7ffffffeull};
    CallMergeArgs a{};
    a.stream = c->reads.d_cigar;
    a.soff = c->reads.d_off64;
    a.rec = c->reads.d_rec;
    a.n_reads = (uint64_t)c->n_reads;
    a.gap = gap;
    a.min_len = min_len;
    // short reads (fewer than 64 ops a read on average, the index build's own test): four reads a wave
    const bool team16 = c->n_ops <= 64ull * a.n_reads;
    const uint64_t waves = team16 ? (a.n_reads + 3) / 4 : a.n_reads;
    const dim3 grid((unsigned)((waves + WPB - 1) / WPB)), block(64 * WPB);
    uint64_t tot[CM_NSTAT];
    m.stats = svt_call_merge_stats{};
    const svt_status s = callindex_build(
        c, m, text, tot, &m.stats.build_ms,
        [&](const BkFile &f) {
            a.f = f;
            if (team16) hipLaunchKernelGGL((callmerge_kernel<true, 16>), grid, block, 0, nullptr, a);
            else hipLaunchKernelGGL((callmerge_kernel<true, WAVE>), grid, block, 0, nullptr, a);
        },
        [](const uint64_t *t) { return CallIndexExpect{t[3], 0, t[3]}; },
        [&](const BkFile &f) {
            a.f = f;
            if (team16) hipLaunchKernelGGL((callmerge_kernel<false, 16>), grid, block, 0, nullptr, a);
            else hipLaunchKernelGGL((callmerge_kernel<false, WAVE>), grid, block, 0, nullptr, a);
        });
    if (s) return s;
    m.stats.fragments = tot[0];
    m.stats.runs = tot[1];
    m.stats.joined_items = tot[2];
    m.stats.items = tot[3];
    m.gap = gap;
    m.min_len = min_len;
    return SVT_OK;
}

}  // namespace
}  // extern "C++"
