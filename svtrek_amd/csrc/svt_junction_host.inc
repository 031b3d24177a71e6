// svt_junction_host.inc -- include/svtrek_junction.h's entry points and the build of the union index
// (included by svt_engine.hip inside its extern "C" block after svt_call_host.inc, whose scan calls
// junction_build and whose CallView names the base view; the kernels are svt_junction.inc).

extern "C++" {
namespace {

// The union index of the loaded pileup, its table and the base view (gap == 0: the plain buckets,
// else the merged index, already built for (gap, min_len)): kept until one of them changes, built here
// otherwise by callindex_build -- the base view's extents added to the counts, the base events copied
// before the junction events are filed behind them.
svt_status junction_build(svt_ctx *c, uint32_t gap, uint32_t min_len) {
    CallScratch::Junction &j = c->call.jn;
    if (gap == 0u) min_len = 0u;   // (ignored without a gap)
    if (j.built && j.gap == gap && j.min_len == min_len) return SVT_OK;
    static const CallIndexText text{"svt_call_scan: the junction index",
                                    "svt_call_scan: more than 2^31 - 1 events with the junction items are not supported",
                                    "junction index build", 0x7fffffffull};
    const CallView base = call_view(c, gap != 0u, false);
    JunctionArgs a{};
    a.off = j.d_toff;
    a.seg = j.d_tseg;
    a.n = j.n;
    a.boff = base.bk.off;
    const dim3 grid((unsigned)((a.n + 64 * WPB - 1) / (64 * WPB))), block(64 * WPB);
    uint64_t tot[JN_NSTAT];
    j.stats = svt_call_junction_stats{};
    const svt_status s = callindex_build(
        c, j, text, tot, &j.stats.build_ms,
        [&](const BkFile &f) {
            a.f = f;
            if (a.n) hipLaunchKernelGGL(junction_kernel<true>, grid, block, 0, nullptr, a);
            hipLaunchKernelGGL(junction_extent_kernel, dim3((unsigned)((2 * f.nbk + 255) / 256)), dim3(256), 0, nullptr, a.boff, f.off,
                               f.nbk);
        },
        [&](const uint64_t *t) { return CallIndexExpect{base.n_s + base.n_i + t[1] + t[2], base.n_s + t[1], base.n_s + t[1]}; },
        [&](const BkFile &f) {
            a.f = f;
            if (base.n_s + base.n_i) {
                const uint64_t waves = 2 * ((f.nbk + WAVE - 1) / WAVE);
                hipLaunchKernelGGL(junction_copy_kernel, dim3((unsigned)((waves + WPB - 1) / WPB)), dim3(64 * WPB), 0, nullptr,
                                   base.bk.ev, a.boff, f.off, f.nbk, f.ev, f.n_ev, f.err);
            }
            if (a.n) hipLaunchKernelGGL(junction_kernel<false>, grid, block, 0, nullptr, a);
        });
    if (s) return s;
    j.stats.records = j.n;
    j.stats.segments = j.rows;
    j.stats.junctions = tot[0];
    j.stats.del_items = tot[1];
    j.stats.ins_items = tot[2];
    j.stats.other = tot[3];
    j.stats.skipped = tot[4];
    j.gap = gap;
    j.min_len = min_len;
    return SVT_OK;
}

svt_status junction_load_1(svt_ctx *c, const svt_junction_view *v) {
    const uint64_t n = v->n, nr = (uint64_t)c->n_reads;
    if (n && (!v->read || !v->off)) return fail(c, SVT_EINVAL, "%s", "svt_load_junctions: null read/off");
    if (n > nr) return fail(c, SVT_EINVAL, "%s", "svt_load_junctions: more records than the pileup has reads");
    const uint64_t rows = n ? v->off[n] : 0;
    if (n && v->off[0] != 0) return fail(c, SVT_EINVAL, "%s", "svt_load_junctions: off[0] != 0");
    if (rows && !v->seg) return fail(c, SVT_EINVAL, "%s", "svt_load_junctions: null seg");
    for (uint64_t k = 0; k < n; k++) {
        if (v->read[k] >= nr || (k && v->read[k] <= v->read[k - 1]))
            return fail(c, SVT_EINVAL, "%s", "svt_load_junctions: read not strictly ascending or past the pileup");
        if (v->off[k + 1] <= v->off[k] || v->off[k + 1] > rows)
            return fail(c, SVT_EINVAL, "%s", "svt_load_junctions: off not monotone, or a record with no row");
    }
    for (uint64_t r = 0; r < rows; r++) {
        const svt_junction_seg &g = v->seg[r];
        if (g.strand > 1u || g.r_end < g.r_beg || g.q_end < g.q_beg || g.tid < 0 || g.tid >= c->n_targets)
            return fail(c, SVT_EINVAL, "%s", "svt_load_junctions: a segment with strand > 1, r_end < r_beg, q_end < q_beg or tid outside the targets");
    }
    if (n) {   // the own segments against the pileup's records
        std::vector<uint4> rec((size_t)nr);
        HIP_TRY(c, hipMemcpy(rec.data(), c->reads.d_rec, (size_t)nr * sizeof(uint4), hipMemcpyDeviceToHost));
        for (uint64_t k = 0; k < n; k++) {
            const svt_junction_seg &g = v->seg[v->off[k]];
            const uint4 &q = rec[(size_t)v->read[k]];
            if ((uint32_t)g.tid != q.w || g.r_beg != q.x || (g.r_end != q.y && !(g.r_end == q.x && q.y == q.x + 1u)))   // (bam_endpos: pos + 1 for no reference base)
                return fail(c, SVT_EINVAL, "%s", "svt_load_junctions: an own segment is not its pileup record's contig / pos / endpos");
        }
    }
    CallScratch::Junction &j = c->call.jn;
    DevBuf<uint64_t> d_toff;
    DevBuf<svt_junction_seg> d_tseg;
    svt_status s;
    if ((s = nomem(c, d_toff.reserve(n + 1), "svt_load_junctions: device buffers")) ||
        (s = nomem(c, d_tseg.reserve(std::max<uint64_t>(rows, 1)), "svt_load_junctions: device buffers")))
        return s;
    const uint64_t zero = 0;
    HIP_TRY(c, hipMemcpy(d_toff, n ? v->off : &zero, (size_t)(n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
    if (rows) HIP_TRY(c, hipMemcpy(d_tseg, v->seg, (size_t)rows * sizeof(svt_junction_seg), hipMemcpyHostToDevice));
    CallScratch::Rearr &rr = c->call.rr;
    if (j.built || rr.built || c->call.bn.built) HIP_TRY(c, hipDeviceSynchronize());
    j.drop();    // the union, the rearrangement index and the breakend list of the table before: gone with it
    rr.drop();
    c->call.bn.drop();
    j.d_toff = std::move(d_toff);
    j.d_tseg = std::move(d_tseg);
    j.n = n;
    j.rows = rows;
    j.loaded = true;
    return SVT_OK;
}

}  // namespace
}  // extern "C++"

svt_status svt_load_junctions(svt_ctx *c, const svt_junction_view *v) {
    if (!c) return SVT_EINVAL;
    if (!v) return fail(c, SVT_EINVAL, "%s", "null view");
    if (!c->loaded) return fail(c, SVT_ESTATE, "%s", "svt_load_pileup not called");
    DEV_GUARD(c);
    return junction_load_1(c, v);
}

svt_status svt_call_junction_stats_get(const svt_ctx *c, svt_call_junction_stats *out) {
    if (!c || !out) return SVT_EINVAL;
    *out = c->call.last.junction_stats;
    return SVT_OK;
}
