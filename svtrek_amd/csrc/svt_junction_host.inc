// svt_junction_host.inc -- include/svtrek_junction.h's entry points and the build of the union index
// (included by svt_engine.hip inside its extern "C" block after svt_call_host.inc, whose scan calls
// junction_build and whose CallView names the base view; the kernels are svt_junction.inc).

extern "C++" {
namespace {

constexpr const char *JN_MEM = "svt_call_scan: the junction index";

// The union index of the loaded pileup, its table and the base view (gap == 0: the plain buckets,
// else the merged index, already built for (gap, min_len)): kept until one of them changes, built here
// otherwise -- the counting pass, the extents (the base view's added, an exclusive sum per row), the
// copy of the base events, the filing pass.
svt_status junction_build(svt_ctx *c, uint32_t gap, uint32_t min_len) {
    CallScratch::Junction &j = c->call.jn;
    if (gap == 0u) min_len = 0u;   // (ignored without a gap)
    if (j.built && j.gap == gap && j.min_len == min_len) return SVT_OK;
    j.built = j.ready = false;
    j.n_seg = 0;
    j.events[0] = j.events[1] = 0;
    j.stats = svt_call_junction_stats{};
    const CallView base = call_view(c, gap != 0u, false);
    const uint64_t S1 = c->bk_n + 1;
    svt_status s;
    DevBuf<uint32_t> d_cur;
    DevBuf<unsigned long long> d_stat;
    DevBuf<uint8_t> d_tmp;
    constexpr size_t NST = (size_t)JN_NSTAT * JN_SLOTS;
    if ((s = nomem(c, j.d_off.reserve(BA_N * S1), JN_MEM)) || (s = nomem(c, d_cur.reserve(2 * S1), JN_MEM)) ||
        (s = nomem(c, d_stat.reserve(NST + 1), JN_MEM)))
        return s;
    DevEvent e0, e1;
    HIP_TRY(c, e0.create());
    HIP_TRY(c, e1.create());
    HIP_TRY(c, hipEventRecord(e0, nullptr));
    HIP_TRY(c, hipMemsetAsync(j.d_off, 0, BA_N * S1 * sizeof(uint32_t), nullptr));
    HIP_TRY(c, hipMemsetAsync(d_cur, 0, 2 * S1 * sizeof(uint32_t), nullptr));
    HIP_TRY(c, hipMemsetAsync(d_stat, 0, (NST + 1) * sizeof(unsigned long long), nullptr));
    JunctionArgs a{};
    a.off = j.d_toff;
    a.seg = j.d_tseg;
    a.n = j.n;
    a.cbase = c->d_bkbase;
    a.cnb = c->d_bknb;
    a.nbk = c->bk_n;
    a.boff = base.bk.off;
    a.uoff = j.d_off;
    a.cur = d_cur;
    a.stat = d_stat;
    a.err = reinterpret_cast<uint32_t *>(d_stat + NST);
    const dim3 jgrid((unsigned)((a.n + 64 * WPB - 1) / (64 * WPB))), jblock(64 * WPB);
    if (a.n) hipLaunchKernelGGL(junction_kernel<true>, jgrid, jblock, 0, nullptr, a);
    hipLaunchKernelGGL(junction_extent_kernel, dim3((unsigned)((2 * c->bk_n + 255) / 256)), dim3(256), 0, nullptr, a.boff, a.uoff,
                       a.nbk);
    HIP_TRY(c, hipGetLastError());
    std::vector<unsigned long long> st(NST);
    HIP_TRY(c, hipMemcpy(st.data(), d_stat, NST * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    uint64_t tot[JN_NSTAT] = {};
    for (uint32_t i = 0; i < JN_SLOTS; i++)
        for (int q = 0; q < JN_NSTAT; q++) tot[q] += st[(size_t)JN_NSTAT * i + q];
    const uint64_t N = base.n_s + base.n_i + tot[1] + tot[2];
    if (N > 0x7fffffffull) return fail(c, SVT_ESTATE, "%s", "svt_call_scan: more than 2^31 - 1 events with the junction items are not supported");
    // the extents: row S from 0, row I behind it (the counts' slot nbk is zero: the row's end)
    uint32_t *offS = j.d_off + (size_t)BA_S * S1, *offI = j.d_off + (size_t)BA_I * S1;
    size_t tb = 0;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveScan(nullptr, tb, offS, offS, hipcub::Sum(), 0u, (int)S1, nullptr));
    if ((s = nomem(c, d_tmp.reserve(tb), JN_MEM))) return s;
    size_t t1 = d_tmp.cap();
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveScan(d_tmp.get(), t1, offS, offS, hipcub::Sum(), 0u, (int)S1, nullptr));
    uint32_t nS = 0;
    HIP_TRY(c, hipMemcpy(&nS, offS + c->bk_n, 4, hipMemcpyDeviceToHost));
    t1 = d_tmp.cap();
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveScan(d_tmp.get(), t1, offI, offI, hipcub::Sum(), nS, (int)S1, nullptr));
    const uint32_t nev = (uint32_t)N;
    if ((uint64_t)nS != base.n_s + tot[1]) return fail(c, SVT_EDEVICE, "%s", "junction index build: the counts disagree");
    if ((s = nomem(c, j.d_ev.reserve(std::max<uint32_t>(nev, 1u)), JN_MEM))) return s;
    a.ev = j.d_ev;
    a.n_ev = nev;
    if (base.n_s + base.n_i) {
        const uint64_t waves = 2 * ((c->bk_n + WAVE - 1) / WAVE);
        hipLaunchKernelGGL(junction_copy_kernel, dim3((unsigned)((waves + WPB - 1) / WPB)), dim3(64 * WPB), 0, nullptr, base.bk.ev,
                           a.boff, j.d_off.get(), a.nbk, a.ev, nev, a.err);
    }
    if (a.n) hipLaunchKernelGGL(junction_kernel<false>, jgrid, jblock, 0, nullptr, a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(e1, nullptr));
    HIP_TRY(c, hipEventSynchronize(e1));
    uint32_t err = 0;
    HIP_TRY(c, hipMemcpy(&err, a.err, 4, hipMemcpyDeviceToHost));
    if (err) return fail(c, SVT_EDEVICE, "%s", "junction index build: the filing disagrees with its count");
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, e0, e1));
    j.events[0] = nS;
    j.events[1] = nev - nS;
    j.stats.records = j.n;
    j.stats.segments = j.rows;
    j.stats.junctions = tot[0];
    j.stats.del_items = tot[1];
    j.stats.ins_items = tot[2];
    j.stats.other = tot[3];
    j.stats.skipped = tot[4];
    j.stats.build_ms = ms;
    j.gap = gap;
    j.min_len = min_len;
    j.built = true;
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
        HIP_TRY(c, hipMemcpy(rec.data(), c->d_rec, (size_t)nr * sizeof(uint4), hipMemcpyDeviceToHost));
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
    if (j.built || j.ready) {   // the index of the table before: gone with it
        HIP_TRY(c, hipDeviceSynchronize());
        j.d_ev.reset();
        j.d_off.reset();
        j.d_seg.reset();
    }
    j.built = j.ready = false;
    CallScratch::Rearr &rr = c->call.rr;   // the rearrangement index of the table before (svt_rearr_host.inc): likewise
    if (rr.built || rr.ready) {
        HIP_TRY(c, hipDeviceSynchronize());
        rr.d_ev.reset();
        rr.d_off.reset();
        rr.d_seg.reset();
    }
    rr.built = rr.ready = false;
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
    *out = c->call.junction;
    return SVT_OK;
}
