// svt_bnd_host.inc -- include/svtrek_bnd.h's entry point, the build of the BND item list and the scan's
// BND stage (included by svt_engine.hip inside its extern "C" block after svt_rearr_host.inc;
// svt_call_host.inc's scan calls bnd_build and bnd_stage; the kernels are svt_bnd.inc).

extern "C++" {
namespace {

constexpr const char *BND_MEM = "svt_call_scan: the breakend list";

// Bits a value below `n` needs (at least 1).
int bnd_bits(uint64_t n) {
    int b = 1;
    while (b < 64 && (n - 1) >> b) b++;
    return n > 1 ? b : 1;
}

// One stable radix pass over bits [b0, b1) of the keys, the values beside them.
template <typename V>
svt_status bnd_sort(svt_ctx *c, const unsigned long long *kin, unsigned long long *kout, const V *vin, V *vout, uint32_t n, int b0,
                    int b1) {
    DevBuf<uint8_t> &tmp = c->call.d_tmp;
    size_t tb = 0;
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, tb, kin, kout, vin, vout, (int)n, b0, b1, nullptr));
    if (svt_status s = nomem(c, tmp.reserve(tb), BND_MEM)) return s;
    tb = tmp.cap();
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(tmp.get(), tb, kin, kout, vin, vout, (int)n, b0, b1, nullptr));
    return SVT_OK;
}

// marks[0 .. n) to their inclusive sum in place; *last = the sum (the number of marks).
svt_status bnd_number(svt_ctx *c, uint32_t *marks, uint32_t n, uint32_t *last) {
    DevBuf<uint8_t> &tmp = c->call.d_tmp;
    size_t tb = 0;
    HIP_TRY(c, hipcub::DeviceScan::InclusiveSum(nullptr, tb, marks, marks, (int)n, nullptr));
    if (svt_status s = nomem(c, tmp.reserve(tb), BND_MEM)) return s;
    tb = tmp.cap();
    HIP_TRY(c, hipcub::DeviceScan::InclusiveSum(tmp.get(), tb, marks, marks, (int)n, nullptr));
    HIP_TRY(c, hipMemcpy(last, marks + (n - 1), 4, hipMemcpyDeviceToHost));
    return SVT_OK;
}

// The item list of the loaded pileup's table: kept until the table changes (svt_load_junctions drops it),
// built here otherwise -- one appending pass, the sort on x, the sort on the class word's bits in use
// (tid_hi << 2 | o, then tid_lo: no pass over the zero bits between them), the count of the classes.
svt_status bnd_build(svt_ctx *c) {
    CallScratch::Bnd &b = c->call.bn;
    const CallScratch::Junction &j = c->call.jn;
    if (b.built) return SVT_OK;
    b.drop();
    const uint64_t n = j.n;
    if (n > 0x7fffffffull) return fail(c, SVT_ESTATE, "%s", "svt_call_scan: more than 2^31 - 1 table records are not supported with bnd = 1");
    svt_status s;
    if ((s = nomem(c, b.d_ctr.reserve(4), BND_MEM))) return s;
    DevEvent e0, e1;
    HIP_TRY(c, e0.create());
    HIP_TRY(c, e1.create());
    HIP_TRY(c, hipEventRecord(e0, nullptr));
    HIP_TRY(c, hipMemsetAsync(b.d_ctr, 0, 4 * sizeof(uint32_t), nullptr));
    uint32_t ctr[2] = {0, 0}, classes = 0;
    if (n) {
        if ((s = nomem(c, b.d_cls.reserve(n), BND_MEM)) || (s = nomem(c, b.d_xy.reserve(n), BND_MEM))) return s;
        const BndBuild a{j.d_toff, j.d_tseg, n, b.d_cls, b.d_xy, b.d_ctr};
        hipLaunchKernelGGL(bnd_kernel, dim3((unsigned)((n + 64 * WPB - 1) / (64 * WPB))), dim3(64 * WPB), 0, nullptr, a);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpy(ctr, b.d_ctr, sizeof ctr, hipMemcpyDeviceToHost));
        if ((uint64_t)ctr[0] + ctr[1] > n) return fail(c, SVT_EDEVICE, "%s", "breakend list build: more items than table records");
    }
    const uint32_t m = ctr[0];
    if (m) {
        DevBuf<unsigned long long> cls2, xy2;   // the sorts' other halves
        if ((s = nomem(c, cls2.reserve(m), BND_MEM)) || (s = nomem(c, xy2.reserve(m), BND_MEM)) || (s = nomem(c, b.d_cid.reserve(m), BND_MEM)))
            return s;
        const int tb = bnd_bits((uint64_t)c->n_targets);
        // by x (keys xy, values cls), then by the class word (keys cls, values xy): the low field, the high field
        if ((s = bnd_sort(c, b.d_xy.get(), xy2.get(), b.d_cls.get(), cls2.get(), m, 32, 32 + BND_XBITS)) ||
            (s = bnd_sort(c, cls2.get(), b.d_cls.get(), xy2.get(), b.d_xy.get(), m, 0, 2 + tb)) ||
            (s = bnd_sort(c, b.d_cls.get(), cls2.get(), b.d_xy.get(), xy2.get(), m, 33, 33 + tb)))
            return s;
        b.d_cls = std::move(cls2);   // (three passes: the ordered list is in the other halves; the n-slot buffers go)
        b.d_xy = std::move(xy2);
        hipLaunchKernelGGL(bnd_head_kernel<0>, dim3((m + 255u) / 256u), dim3(256), 0, nullptr, b.d_cls.get(), b.d_xy.get(), m, BND_SAT,
                           b.d_cid.get());
        HIP_TRY(c, hipGetLastError());
        if ((s = bnd_number(c, b.d_cid.get(), m, &classes))) return s;
    }
    HIP_TRY(c, hipEventRecord(e1, nullptr));
    HIP_TRY(c, hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, e0, e1));
    b.n_items = m;
    b.stats.items = (uint64_t)ctr[0] + ctr[1];
    b.stats.skipped = ctr[1];
    b.stats.classes = classes;
    b.stats.build_ms = ms;
    b.built = true;
    return SVT_OK;
}

// The BND stage of a scan, behind whatever its other passes did: their n_other calls `others` (in order)
// and the BND calls of the built list into k.d_calls; *total = their number.  Adds its counts to the
// scan's stats.
svt_status bnd_stage(svt_ctx *c, const svt_call_params *p, const svt_call *others, uint32_t n_other, uint64_t *total) {
    CallScratch &k = c->call;
    CallScratch::Bnd &b = k.bn;
    const uint32_t m = (uint32_t)b.n_items, link = (uint32_t)p->link;
    const dim3 ig((m + 255u) / 256u), ib(256);
    svt_status s;
    if ((s = nomem(c, b.d_cid.reserve(m), BND_MEM)) || (s = nomem(c, b.d_gid.reserve(m), BND_MEM)) ||
        (s = nomem(c, b.d_key.reserve(m), BND_MEM)) || (s = nomem(c, b.d_key2.reserve(m), BND_MEM)) ||
        (s = nomem(c, b.d_x.reserve(m), BND_MEM)) || (s = nomem(c, b.d_x2.reserve(m), BND_MEM)))
        return s;
    uint32_t ncl = 0, ng = 0, npick = 0;
    hipLaunchKernelGGL(bnd_head_kernel<0>, ig, ib, 0, nullptr, b.d_cls.get(), b.d_xy.get(), m, link, b.d_cid.get());
    HIP_TRY(c, hipGetLastError());
    if ((s = bnd_number(c, b.d_cid.get(), m, &ncl))) return s;
    if (ncl == 0 || ncl > m) return fail(c, SVT_EDEVICE, "%s", "svt_call_scan: the breakends' cluster count is out of range");
    if ((s = nomem(c, b.d_ccls.reserve(ncl), BND_MEM))) return s;
    hipLaunchKernelGGL(bnd_key_kernel, ig, ib, 0, nullptr, b.d_cls.get(), b.d_xy.get(), b.d_cid.get(), m, b.d_key.get(), b.d_x.get(),
                       b.d_ccls.get());
    HIP_TRY(c, hipGetLastError());
    if ((s = bnd_sort(c, b.d_key.get(), b.d_key2.get(), b.d_x.get(), b.d_x2.get(), m, 0, BND_XBITS + bnd_bits(ncl)))) return s;
    hipLaunchKernelGGL(bnd_head_kernel<1>, ig, ib, 0, nullptr, (const unsigned long long *)nullptr, b.d_key2.get(), m, link, b.d_gid.get());
    HIP_TRY(c, hipGetLastError());
    if ((s = bnd_number(c, b.d_gid.get(), m, &ng))) return s;
    if (ng < ncl || ng > m) return fail(c, SVT_EDEVICE, "%s", "svt_call_scan: the breakends' group count is out of range");
    hipcub::CountingInputIterator<uint32_t> it(0);
    uint32_t *d_np = b.d_ctr + 2;
    size_t need = 0;
    HIP_TRY(c, hipcub::DeviceSelect::Flagged(nullptr, need, it, b.d_flag.get(), b.d_pick.get(), d_np, (int)ng, nullptr));
    if ((s = nomem(c, b.d_acc.reserve(ng), BND_MEM)) || (s = nomem(c, b.d_flag.reserve(ng), BND_MEM)) ||
        (s = nomem(c, b.d_pick.reserve(ng), BND_MEM)) || (s = nomem(c, k.d_tmp.reserve(need), BND_MEM)))
        return s;
    HIP_TRY(c, hipMemsetAsync(b.d_acc, 0, (size_t)ng * sizeof(BndAcc), nullptr));
    hipLaunchKernelGGL(bnd_accum_kernel, ig, ib, 0, nullptr, b.d_key2.get(), b.d_x2.get(), b.d_gid.get(), b.d_ccls.get(), m, b.d_acc.get());
    hipLaunchKernelGGL(bnd_pick_kernel, dim3((ng + 255u) / 256u), dim3(256), 0, nullptr, b.d_acc.get(), ng, (uint32_t)p->min_support,
                       b.d_flag.get());
    need = k.d_tmp.cap();
    HIP_TRY(c, hipcub::DeviceSelect::Flagged(k.d_tmp.get(), need, it, b.d_flag.get(), b.d_pick.get(), d_np, (int)ng, nullptr));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpy(&npick, d_np, 4, hipMemcpyDeviceToHost));
    if (npick > ng) return fail(c, SVT_EDEVICE, "%s", "svt_call_scan: the breakends' call count is out of range");
    *total = (uint64_t)n_other + npick;
    if (*total > 0x7fffffffull) return fail(c, SVT_ESTATE, "%s", "svt_call_scan: more than 2^31 - 1 calls are not supported");
    if (npick) {
        if ((s = nomem(c, b.d_raw.reserve(npick), BND_MEM)) || (s = nomem(c, b.d_sorted.reserve(npick), BND_MEM)) ||
            (s = nomem(c, b.d_k.reserve(npick), BND_MEM)) || (s = nomem(c, b.d_k2.reserve(npick), BND_MEM)) ||
            (s = nomem(c, b.d_idx.reserve(npick), BND_MEM)) || (s = nomem(c, b.d_idx2.reserve(npick), BND_MEM)))
            return s;
        const KArgs ka = make_args(c, nullptr, nullptr, 0, false);
        const dim3 cg((npick + 255u) / 256u), cb(256);
        const int cbits = bnd_bits((uint64_t)c->n_targets + 1);   // (a chrom is tid + 1)
        hipLaunchKernelGGL(bnd_emit_kernel, dim3((npick + WPB - 1) / WPB), dim3(64 * WPB), 0, nullptr, ka.pile, b.d_acc.get(),
                           b.d_pick.get(), npick, b.d_raw.get(), b.d_k.get(), b.d_idx.get());
        HIP_TRY(c, hipGetLastError());
        // (mate chrom, o, end), then (chrom, pos): two stable passes on the call indices
        if ((s = bnd_sort(c, b.d_k.get(), b.d_k2.get(), b.d_idx.get(), b.d_idx2.get(), npick, 0, 32 + cbits))) return s;
        hipLaunchKernelGGL(bnd_hikey_kernel, cg, cb, 0, nullptr, b.d_raw.get(), b.d_idx2.get(), npick, b.d_k.get());
        HIP_TRY(c, hipGetLastError());
        if ((s = bnd_sort(c, b.d_k.get(), b.d_k2.get(), b.d_idx2.get(), b.d_idx.get(), npick, 0, 32 + cbits))) return s;
        hipLaunchKernelGGL(bnd_gather_kernel, cg, cb, 0, nullptr, b.d_raw.get(), b.d_idx.get(), npick, b.d_sorted.get());
        HIP_TRY(c, hipGetLastError());
    }
    if ((s = call_merge(c, others, n_other, b.d_sorted.get(), npick, k.d_calls))) return s;
    k.last.call_stats.clusters += ncl;
    k.last.call_stats.calls += npick;
    k.last.bnd_stats.clusters = ncl;
    k.last.bnd_stats.groups = ng;
    k.last.bnd_stats.calls = npick;
    return SVT_OK;
}

}  // namespace
}  // extern "C++"

svt_status svt_call_bnd_stats_get(const svt_ctx *c, svt_call_bnd_stats *out) {
    if (!c || !out) return SVT_EINVAL;
    *out = c->call.last.bnd_stats;
    return SVT_OK;
}
