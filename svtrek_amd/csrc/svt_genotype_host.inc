// svt_genotype_host.inc -- include/svtrek_genotype.h's entry points (included by svt_engine.hip inside
// its extern "C" block after svt_call_host.inc; the kernel is svt_genotype.inc).

extern "C++" {
namespace {

// What every entry point tests before it looks at its buffers.
svt_status gt_check(svt_ctx *c, const svt_gt_params *p, size_t n) {
    if (!p) return fail(c, SVT_EINVAL, "%s", "null params");
    if (p->flank < 0 || p->flank > (1 << 20)) return fail(c, SVT_EINVAL, "%s", "svt_genotype: flank in [0, 2^20]");
    if (n > 0x3fffffffull) return fail(c, SVT_EINVAL, "batch too large (%s)", "n > 2^30-1");
    if (!c->loaded) return fail(c, SVT_ESTATE, "%s", "svt_load_pileup not called");
    if (c->n_reads != 0 && !c->bk.ready)
        return fail(c, SVT_ESTATE, "%s",
                    "svt_genotype needs the value buckets (not built: SVTREK_INDEX=lists, or a pileup past 2^32 events)");
    return SVT_OK;
}

// One launch over n > 0 records of either kind, ordered after the context's earlier launches.
template <typename Site>
svt_status gt_launch(svt_ctx *c, const svt_gt_params *p, const Site *d_sites, size_t n, svt_gt *d_out, hipStream_t st,
                     bool merged = false, bool junction = false) {
    const svt_status s = order_on(c, st);   // (svt_reindex rebuilds the buckets)
    if (s) return s;
    const KArgs ka = make_args(c, nullptr, nullptr, 0, false);
    GtArgs g{};
    g.bk = merged || junction ? call_view(c, merged, junction).bk : ka.bk;   // (svt_genotype_calls after a merged / junction scan: the items it clustered)
    g.pile = ka.pile;
    g.prm = *p;
    g.nt = c->n_reads ? c->n_targets : 0;
    g.n = (uint32_t)n;
    const dim3 grid((unsigned)((n + WPB - 1) / WPB)), block(64 * WPB);
    if (junction) hipLaunchKernelGGL((genotype_kernel<Site, true>), grid, block, 0, st, g, d_sites, d_out);
    else hipLaunchKernelGGL(genotype_kernel<Site>, grid, block, 0, st, g, d_sites, d_out);
    HIP_TRY(c, hipGetLastError());
    return SVT_OK;
}

}  // namespace
}  // extern "C++"

void svt_genotype_default_params(const svt_ctx *, svt_gt_params *out) {
    if (!out) return;
    *out = svt_gt_params{50, 0, {223u, 3010u, 13010u}, {13010u, 3010u, 223u}};
}

svt_status svt_genotype_device(svt_ctx *c, const svt_gt_params *p, const svt_gt_site *d_sites, size_t n, svt_gt *d_out,
                               void *stream) {
    if (!c) return SVT_EINVAL;
    if (svt_status s = gt_check(c, p, n)) return s;
    if (n == 0) return SVT_OK;
    if (!d_sites || !d_out) return fail(c, SVT_EINVAL, "%s", "null sites/out");
    DEV_GUARD(c);
    return gt_launch(c, p, d_sites, n, d_out, (hipStream_t)stream);
}

svt_status svt_genotype_batch(svt_ctx *c, const svt_gt_params *p, const svt_gt_site *sites, size_t n, svt_gt *out) {
    if (!c) return SVT_EINVAL;
    if (svt_status s = gt_check(c, p, n)) return s;
    if (n == 0) return SVT_OK;
    if (!sites || !out) return fail(c, SVT_EINVAL, "%s", "null sites/out");
    DEV_GUARD(c);
    svt_status s;
    if ((s = nomem(c, c->d_gtsite.reserve(n), "svt_genotype_batch: device buffers")) ||
        (s = nomem(c, c->d_gt.reserve(n), "svt_genotype_batch: device buffers")))
        return s;
    HIP_TRY(c, hipMemcpy(c->d_gtsite, sites, n * sizeof(svt_gt_site), hipMemcpyHostToDevice));
    if ((s = gt_launch(c, p, c->d_gtsite.get(), n, c->d_gt.get(), nullptr))) return s;
    HIP_TRY(c, hipStreamSynchronize(nullptr));
    HIP_TRY(c, hipMemcpy(out, c->d_gt, n * sizeof(svt_gt), hipMemcpyDeviceToHost));
    return SVT_OK;
}

svt_status svt_genotype_calls(svt_ctx *c, const svt_gt_params *p, svt_gt *out, uint64_t n_out) {
    if (!c) return SVT_EINVAL;
    if (svt_status s = gt_check(c, p, (size_t)n_out)) return s;
    if (!c->call.scanned) return fail(c, SVT_ESTATE, "%s", "svt_genotype_calls: no svt_call_scan of the loaded pileup");
    if (n_out != c->call.n_calls) return fail(c, SVT_EINVAL, "%s", "svt_genotype_calls: n_out is not the scanned count");
    if (n_out == 0) return SVT_OK;
    if (!out) return fail(c, SVT_EINVAL, "%s", "null out");
    DEV_GUARD(c);
    svt_status s;
    if ((s = nomem(c, c->d_gt.reserve(n_out), "svt_genotype_calls: device buffer"))) return s;
    if ((s = gt_launch(c, p, c->call.d_calls.get(), (size_t)n_out, c->d_gt.get(), nullptr, c->call.last.merged, c->call.last.junction)))
        return s;
    HIP_TRY(c, hipStreamSynchronize(nullptr));
    HIP_TRY(c, hipMemcpy(out, c->d_gt, n_out * sizeof(svt_gt), hipMemcpyDeviceToHost));
    return SVT_OK;
}
