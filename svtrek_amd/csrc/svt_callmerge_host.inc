// svt_callmerge_host.inc -- the build of the merged index (included by svt_engine.hip inside its
// extern "C" block before svt_call_host.inc, whose scan calls it; the kernel is svt_callmerge.inc).

extern "C++" {
namespace {

constexpr const char *CM_MEM = "svt_call_scan: the merged index";

// The merged index of the loaded pileup for (gap, min_len): kept until either changes, built here
// otherwise -- the counting walk, the extents (an exclusive sum per row), the filing walk.
svt_status callmerge_build(svt_ctx *c, uint32_t gap, uint32_t min_len) {
    CallScratch::Merged &m = c->call.mg;
    if (m.built && m.gap == gap && m.min_len == min_len) return SVT_OK;
    m = CallScratch::Merged{};
    const uint64_t S1 = c->bk_n + 1;
    svt_status s;
    DevBuf<uint32_t> d_cur;
    DevBuf<unsigned long long> d_stat;
    DevBuf<uint8_t> d_tmp;
    if ((s = nomem(c, m.d_off.reserve(BA_N * S1), CM_MEM)) || (s = nomem(c, d_cur.reserve(2 * S1), CM_MEM)) ||
        (s = nomem(c, d_stat.reserve(4 * CM_SLOTS + 1), CM_MEM)))
        return s;
    DevEvent e0, e1;
    HIP_TRY(c, e0.create());
    HIP_TRY(c, e1.create());
    HIP_TRY(c, hipEventRecord(e0, nullptr));
    HIP_TRY(c, hipMemsetAsync(m.d_off, 0, BA_N * S1 * sizeof(uint32_t), nullptr));
    HIP_TRY(c, hipMemsetAsync(d_cur, 0, 2 * S1 * sizeof(uint32_t), nullptr));
    HIP_TRY(c, hipMemsetAsync(d_stat, 0, (4 * CM_SLOTS + 1) * sizeof(unsigned long long), nullptr));
    CallMergeArgs a{};
    a.stream = c->d_cigar;
    a.soff = c->d_off64;
    a.rec = c->d_rec;
    a.n_reads = (uint64_t)c->n_reads;
    a.cbase = c->d_bkbase;
    a.cnb = c->d_bknb;
    a.nbk = c->bk_n;
    a.off = m.d_off;
    a.cur = d_cur;
    a.stat = d_stat;
    a.err = reinterpret_cast<uint32_t *>(d_stat + 4 * CM_SLOTS);
    a.gap = gap;
    a.min_len = min_len;
    // short reads (fewer than 64 ops a read on average, the index build's own test): four reads a wave
    const bool team16 = c->n_ops <= 64ull * a.n_reads;
    const uint64_t waves = team16 ? (a.n_reads + 3) / 4 : a.n_reads;
    const dim3 grid((unsigned)((waves + WPB - 1) / WPB)), block(64 * WPB);
    if (team16) hipLaunchKernelGGL((callmerge_kernel<true, 16>), grid, block, 0, nullptr, a);
    else hipLaunchKernelGGL((callmerge_kernel<true, WAVE>), grid, block, 0, nullptr, a);
    HIP_TRY(c, hipGetLastError());
    std::vector<unsigned long long> st(4 * CM_SLOTS + 1);
    HIP_TRY(c, hipMemcpy(st.data(), d_stat, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    uint64_t tot[4] = {};
    for (uint32_t i = 0; i < CM_SLOTS; i++)
        for (int q = 0; q < 4; q++) tot[q] += st[4 * i + q];
    if (tot[3] >= 0x7fffffffull) return fail(c, SVT_ESTATE, "%s", "svt_call_scan: 2^31 merged events and more are not supported");
    // the extents: row S from 0, row I behind it (the counts' slot nbk is zero: the row's end)
    uint32_t *offS = m.d_off + (size_t)BA_S * S1, *offI = m.d_off + (size_t)BA_I * S1;
    size_t tb = 0;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveScan(nullptr, tb, offS, offS, hipcub::Sum(), 0u, (int)S1, nullptr));
    if ((s = nomem(c, d_tmp.reserve(tb), CM_MEM))) return s;
    size_t t1 = d_tmp.cap();
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveScan(d_tmp.get(), t1, offS, offS, hipcub::Sum(), 0u, (int)S1, nullptr));
    uint32_t nS = 0;
    HIP_TRY(c, hipMemcpy(&nS, offS + c->bk_n, 4, hipMemcpyDeviceToHost));
    t1 = d_tmp.cap();
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveScan(d_tmp.get(), t1, offI, offI, hipcub::Sum(), nS, (int)S1, nullptr));
    const uint32_t nev = (uint32_t)tot[3];
    if (nS > nev) return fail(c, SVT_EDEVICE, "%s", "merged index build: the counts disagree");
    if ((s = nomem(c, m.d_ev.reserve(std::max<uint32_t>(nev, 1u)), CM_MEM))) return s;
    a.ev = m.d_ev;
    a.n_ev = nev;
    if (team16) hipLaunchKernelGGL((callmerge_kernel<false, 16>), grid, block, 0, nullptr, a);
    else hipLaunchKernelGGL((callmerge_kernel<false, WAVE>), grid, block, 0, nullptr, a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(e1, nullptr));
    HIP_TRY(c, hipEventSynchronize(e1));
    uint32_t err = 0;
    HIP_TRY(c, hipMemcpy(&err, a.err, 4, hipMemcpyDeviceToHost));
    if (err) return fail(c, SVT_EDEVICE, "%s", "merged index build: the filing disagrees with its count");
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, e0, e1));
    m.events[0] = nS;
    m.events[1] = nev - nS;
    m.stats.fragments = tot[0];
    m.stats.runs = tot[1];
    m.stats.joined_items = tot[2];
    m.stats.items = tot[3];
    m.stats.build_ms = ms;
    m.gap = gap;
    m.min_len = min_len;
    m.built = true;
    return SVT_OK;
}

}  // namespace
}  // extern "C++"
