// svt_rearr_host.inc -- include/svtrek_rearr.h's entry point and the build of the rearrangement index
// (included by svt_engine.hip inside its extern "C" block after svt_junction_host.inc; svt_call_host.inc's
// scan calls rearr_build and runs its second pass over rearr_view; the kernels are svt_rearr.inc).

extern "C++" {
namespace {

constexpr const char *RR_MEM = "svt_call_scan: the rearrangement index";

// The index of the loaded pileup's table: kept until the table changes (svt_load_junctions drops it),
// built here otherwise -- the counting pass, an exclusive sum per row, the filing pass.
svt_status rearr_build(svt_ctx *c) {
    CallScratch::Rearr &r = c->call.rr;
    const CallScratch::Junction &j = c->call.jn;
    if (r.built) return SVT_OK;
    r.ready = false;
    r.n_seg = 0;
    r.events[0] = r.events[1] = 0;
    r.stats = svt_call_rearr_stats{};
    const uint64_t S1 = c->bk_n + 1;
    svt_status s;
    DevBuf<uint32_t> d_cur;
    DevBuf<unsigned long long> d_stat;
    DevBuf<uint8_t> d_tmp;
    constexpr size_t NST = (size_t)RR_NSTAT * JN_SLOTS;
    if ((s = nomem(c, r.d_off.reserve(BA_N * S1), RR_MEM)) || (s = nomem(c, d_cur.reserve(2 * S1), RR_MEM)) ||
        (s = nomem(c, d_stat.reserve(NST + 1), RR_MEM)))
        return s;
    DevEvent e0, e1;
    HIP_TRY(c, e0.create());
    HIP_TRY(c, e1.create());
    HIP_TRY(c, hipEventRecord(e0, nullptr));
    HIP_TRY(c, hipMemsetAsync(r.d_off, 0, BA_N * S1 * sizeof(uint32_t), nullptr));
    HIP_TRY(c, hipMemsetAsync(d_cur, 0, 2 * S1 * sizeof(uint32_t), nullptr));
    HIP_TRY(c, hipMemsetAsync(d_stat, 0, (NST + 1) * sizeof(unsigned long long), nullptr));
    RearrArgs a{};
    a.off = j.d_toff;
    a.seg = j.d_tseg;
    a.n = j.n;
    a.cbase = c->d_bkbase;
    a.cnb = c->d_bknb;
    a.nbk = c->bk_n;
    a.roff = r.d_off;
    a.cur = d_cur;
    a.stat = d_stat;
    a.err = reinterpret_cast<uint32_t *>(d_stat + NST);
    const dim3 grid((unsigned)((a.n + 64 * WPB - 1) / (64 * WPB))), block(64 * WPB);
    if (a.n) hipLaunchKernelGGL(rearr_kernel<true>, grid, block, 0, nullptr, a);
    HIP_TRY(c, hipGetLastError());
    std::vector<unsigned long long> st(NST);
    HIP_TRY(c, hipMemcpy(st.data(), d_stat, NST * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    uint64_t tot[RR_NSTAT] = {};
    for (uint32_t i = 0; i < JN_SLOTS; i++)
        for (int q = 0; q < RR_NSTAT; q++) tot[q] += st[(size_t)RR_NSTAT * i + q];
    const uint64_t N = tot[0] + tot[1];   // (at most the table's records: svt_load_junctions bounds them by the reads)
    if (N > 0x7fffffffull) return fail(c, SVT_ESTATE, "%s", "svt_call_scan: more than 2^31 - 1 rearrangement items are not supported");
    // the extents: row S from 0, row I behind it (the counts' slot nbk is zero: the row's end)
    uint32_t *offS = r.d_off + (size_t)BA_S * S1, *offI = r.d_off + (size_t)BA_I * S1;
    size_t tb = 0;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveScan(nullptr, tb, offS, offS, hipcub::Sum(), 0u, (int)S1, nullptr));
    if ((s = nomem(c, d_tmp.reserve(tb), RR_MEM))) return s;
    size_t t1 = d_tmp.cap();
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveScan(d_tmp.get(), t1, offS, offS, hipcub::Sum(), 0u, (int)S1, nullptr));
    uint32_t nS = 0;
    HIP_TRY(c, hipMemcpy(&nS, offS + c->bk_n, 4, hipMemcpyDeviceToHost));
    t1 = d_tmp.cap();
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveScan(d_tmp.get(), t1, offI, offI, hipcub::Sum(), nS, (int)S1, nullptr));
    const uint32_t nev = (uint32_t)N;
    if ((uint64_t)nS != tot[0]) return fail(c, SVT_EDEVICE, "%s", "rearrangement index build: the counts disagree");
    if ((s = nomem(c, r.d_ev.reserve(std::max<uint32_t>(nev, 1u)), RR_MEM))) return s;
    a.ev = r.d_ev;
    a.n_ev = nev;
    if (a.n && nev) hipLaunchKernelGGL(rearr_kernel<false>, grid, block, 0, nullptr, a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(e1, nullptr));
    HIP_TRY(c, hipEventSynchronize(e1));
    uint32_t err = 0;
    HIP_TRY(c, hipMemcpy(&err, a.err, 4, hipMemcpyDeviceToHost));
    if (err) return fail(c, SVT_EDEVICE, "%s", "rearrangement index build: the filing disagrees with its count");
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, e0, e1));
    r.events[0] = nS;
    r.events[1] = nev - nS;
    r.stats.dup_items = tot[0];
    r.stats.inv_items = tot[1];
    r.stats.build_ms = ms;
    r.built = true;
    return SVT_OK;
}

}  // namespace
}  // extern "C++"

svt_status svt_call_rearr_stats_get(const svt_ctx *c, svt_call_rearr_stats *out) {
    if (!c || !out) return SVT_EINVAL;
    *out = c->call.rearr;
    return SVT_OK;
}
