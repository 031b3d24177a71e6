// svt_load_host.inc -- the pileup load and the index builds (included by svt_engine.hip inside its
// extern "C" block): svt_load_pileup, load_core for the BAM decoder's load (svt_bam_host.inc), the
// span-list build, the value buckets' first build, svt_reindex, svt_last_load_stats.  The host pass
// is svt_loadprep.h, the kernels svt_index.inc, svt_index2.inc and svt_bucket_build.inc, the three
// owners of what a load leaves on the device (ReadCols, SpanIndex, ValueBuckets) svt_devmem.inc.

extern "C++" {
namespace {

static_assert(sizeof(loadprep::Rec) == sizeof(uint4) && offsetof(loadprep::Rec, pos) == offsetof(uint4, x) &&
              offsetof(loadprep::Rec, endpos) == offsetof(uint4, y) && offsetof(loadprep::Rec, nc) == offsetof(uint4, z) &&
              offsetof(loadprep::Rec, tid) == offsetof(uint4, w), "the host pass's record is DevPileup's uint4");
static_assert(sizeof(loadprep::Bkt) == sizeof(uint2) && offsetof(loadprep::Bkt, by_pos) == offsetof(uint2, x) &&
              offsetof(loadprep::Bkt, by_emax) == offsetof(uint2, y), "the host pass's read bucket is DevPileup's uint2");

// The host pass's limits from the engine's constants.  Index ranges of ~n_ops / ix_ranges ops, between
// 2048 and 65 536: 32 768 ranges of at most 65 536 ops gave cfg2 index 0.602 -> 0.531 ms, cfg3 2.30 ->
// 2.19 ms against 131 072 ranges (profiles/r05_J; fewer, longer ranges cross fewer range-boundary
// slots), while cfg5's 9 G ops keep ~137 K ranges (the stage's 96 events a range).  A 64-read group of
// the lane-per-read index holds fewer than 2^27 ops.  At most 16 threads.
loadprep::Limits load_limits(const svt_ctx *c) {
    return loadprep::Limits{BKT_SHIFT, NCIG_MASK, OP_SOFT, WAVE, (int64_t)IX_RCAP, 2048, 65536, c->ix_ranges, 1ull << 27, 16};
}

using LoadClock = std::chrono::steady_clock;
double ms_since(LoadClock::time_point a) { return std::chrono::duration<double, std::milli>(LoadClock::now() - a).count(); }

// The device index of the loaded pileup (svt_index.inc / svt_index2.inc).  Stream walk: the walk
// (one pass over the stream, events staged per range), an exclusive scan of the range totals, the
// staged rows to their places.  Lane per read: census, the scan of the group totals, emit.
// `first`: between scan and placement, size and allocate the event lists from the totals (one
// synchronous read-back); later calls (svt_reindex) reuse them -- the totals depend on the
// pileup only.  `ms`: the index kernels' device time (HIP events; read-back and allocations
// excluded).
// lane per read (svt_index2.inc) for short reads -- a wave's 64 reads then take a few steps
// each; long reads (a lane walking thousands of ops waits on its loads) take the stream walk,
// which spreads every slot of 256 ops over the wave; never for a group of > 2^27 ops
bool index_lane(const svt_ctx *c, uint64_t nops, uint64_t nreads) {
    return c->ix.n_groups > 0 && (c->ix_mode == 1 || (c->ix_mode == 0 && nops <= 64ull * nreads));
}

// (what the builds read comes from the owners' views; what they write, from the owners' buffers)
IxArgs ix_args(const svt_ctx *c) {
    const DevPileup v = pile_view(c);
    const SpanIndex &x = c->ix;
    IxArgs a;
    a.stream = v.cigar;
    a.soff = v.off64;
    a.rec = v.rec;
    a.clip8 = c->reads.d_clip8;
    a.part = x.d_part;
    a.agg = x.d_agg;
    a.bsum = x.d_bsum;
    a.bpre = x.d_bpre;
    a.spoffD = x.d_spoffD;
    a.spoffI = x.d_spoffI;
    a.spD = x.d_spD;
    a.spI = x.d_spI;
    a.capD = x.n_evD;
    a.capI = x.n_evI;
    a.err = &ctl(c)->ix_status;   // (svt_sync reports it)
    a.scr = x.d_scr;
    a.scrh = x.d_scrh;
    a.ovf = x.d_ovf;
    a.n_ranges = x.n_ranges;
    return a;
}

svt_status build_index(svt_ctx *c, hipStream_t st, bool first, double *ms) {
    SpanIndex &x = c->ix;
    IxArgs a = ix_args(c);
    DevEvent ev[4];
    if (ms)
        for (auto &e : ev) HIP_TRY(c, e.create());
    const bool lane = index_lane(c, c->n_ops, (uint64_t)c->n_reads);
    c->load_stats.index_kind = lane ? 1u : 2u;
    const uint32_t nparts = lane ? x.n_groups : x.n_ranges;   // what the scan runs over
    Ix2Args a2{a, x.d_cnt, (uint64_t)c->n_reads, x.n_groups};
    const dim3 grid2((unsigned)((x.n_groups + IX2_WPB - 1) / IX2_WPB)), block2(64 * IX2_WPB);
    const dim3 grid1((unsigned)((x.n_ranges + IX_WPB - 1) / IX_WPB)), block1(64 * IX_WPB);
    if (ms) HIP_TRY(c, hipEventRecord(ev[0], st));
    if (x.bsum_dirty) {
        HIP_TRY(c, hipMemsetAsync(x.d_bsum, 0, x.n_bsum * sizeof(IxTot), st));
        x.bsum_dirty = false;
    }
    x.bsum_dirty = true;
    if (lane)
        hipLaunchKernelGGL(ix2_census_kernel, grid2, block2, 0, st, a2);
    else
        hipLaunchKernelGGL(index_kernel, grid1, block1, 0, st, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {   // the blocks' exclusive prefixes (ix_part_base adds the ranges' within a block)
        hipLaunchKernelGGL(ix_scan_blocks_kernel, dim3(1), dim3(IX_SCAN_T), 0, st, x.d_bsum, x.d_bpre,
                           (nparts + IX_BLK - 1) / IX_BLK, x.d_tot, x.d_spoffD, x.d_spoffI, (uint64_t)c->n_reads);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(c, SVT_EDEVICE, "index census: %s", hipGetErrorString(e));
    x.bsum_dirty = false;   // the scan launched: it zeroes the block sums behind itself
    if (ms) HIP_TRY(c, hipEventRecord(ev[1], st));
    if (first) {
        uint64_t t[IX_NTOT];
        e = hipMemcpyAsync(t, x.d_tot, sizeof t, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(c, SVT_EDEVICE, "index totals: %s", hipGetErrorString(e));
        x.n_evD = t[IX_D];
        x.n_evI = t[IX_I];
        c->n_ins = t[IX_I];
        svt_status s;
        if ((s = upload<uint4>(c, x.d_spD, nullptr, 0, std::max<uint64_t>(x.n_evD, 1)))) return s;
        if ((s = upload<uint4>(c, x.d_spI, nullptr, 0, std::max<uint64_t>(x.n_evI, 1)))) return s;
        a = ix_args(c);
        a2.a = a;
    }
    if (ms) HIP_TRY(c, hipEventRecord(ev[2], st));
    if (lane) hipLaunchKernelGGL(ix2_emit_kernel, grid2, block2, 0, st, a2);
    else hipLaunchKernelGGL(ix_copy_kernel, grid1, block1, 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(c, SVT_EDEVICE, "index emit: %s", hipGetErrorString(e));
    if (ms) {
        float t0 = 0.f, t1 = 0.f;
        e = hipEventRecord(ev[3], st);
        if (e == hipSuccess) e = hipEventSynchronize(ev[3]);
        if (e == hipSuccess) e = hipEventElapsedTime(&t0, ev[0], ev[1]);
        if (e == hipSuccess) e = hipEventElapsedTime(&t1, ev[2], ev[3]);
        if (e != hipSuccess) return fail(c, SVT_EDEVICE, "index timing: %s", hipGetErrorString(e));
        *ms = (double)t0 + (double)t1;
    }
    return SVT_OK;
}

// ---- the value-bucketed event index (svt_bucket_build.inc): launch arguments, one pass, the
// first build at load
BkBuild bk_args(const svt_ctx *c, bool count, bool captured) {
    const ValueBuckets &k = c->bk;
    const BkIndex v = k.view();
    BkBuild b{};
    b.ev = k.d_ev;
    b.off = v.off;
    b.cur = count ? k.d_off : captured ? k.d_cap : k.d_cur;
    b.pmx = k.d_pm;
    b.nbk = v.nbk;
    b.maxd = k.d_maxd;
    b.cbase = v.cbase;
    b.cnb = v.cnb;
    b.k = count || captured ? 0u : k.builds;
    b.n_ev = k.nev;
    b.err = &ctl(c)->ix_status;   // (svt_sync reports it)
    return b;
}

// One counting or filing pass on st: short reads walked from the CIGAR stream; long reads counted
// from the span lists (at load) and filed from the stream walk's stage (index_kernel, which the
// caller ran first).
svt_status bk_pass(svt_ctx *c, hipStream_t st, bool count, bool captured) {
    const IxArgs a = ix_args(c);
    const BkBuild b = bk_args(c, count, captured);
    const uint64_t nr = (uint64_t)c->n_reads;
    if (index_lane(c, c->n_ops, nr)) {
        const dim3 grid((unsigned)((c->ix.n_groups + IXB_WPB - 1) / IXB_WPB)), block(64 * IXB_WPB);
        if (count) hipLaunchKernelGGL(ixb_lane_kernel<true>, grid, block, 0, st, a, b, nr);
        else hipLaunchKernelGGL(ixb_lane_kernel<false>, grid, block, 0, st, a, b, nr);
    } else if (count) {   // (at load: the span lists the first build made)
        const dim3 grid((unsigned)((nr + IXB_T - 1) / IXB_T)), block(IXB_T);
        hipLaunchKernelGGL(ixb_lists_kernel<true>, grid, block, 0, st, a, b, nr);
    } else {              // from the stream walk's stage (index_kernel ran just before on st)
        const dim3 grid((unsigned)((c->ix.n_ranges + IX_WPB - 1) / IX_WPB)), block(64 * IX_WPB);
        hipLaunchKernelGGL(ixb_copy_kernel, grid, block, 0, st, a, b);
    }
    HIP_TRY(c, hipGetLastError());
    return SVT_OK;
}

svt_status bk_check_err(svt_ctx *c) {
    uint32_t e = 0;
    HIP_TRY(c, hipDeviceSynchronize());
    if (svt_status s = take_ix_status(c, &e)) return s;
    if (e) return fail(c, SVT_EDEVICE, "%s", "device index build: the value buckets disagree with their count");
    return SVT_OK;
}

// The first build (svt_load_pileup, after the span lists): buckets per contig from the largest
// pos / endpos (values past them -- walks lengthened by H / P / N ops -- share the contig's last
// bucket), the counting pass, the extents and prefix maxima on the host, the filing pass.  A pileup
// whose events or buckets pass 2^32 keeps the span lists alone (bk.ready stays false).
svt_status bk_load(svt_ctx *c, const std::vector<int64_t> &vtop) {
    ValueBuckets &k = c->bk;
    const int32_t nt = c->n_targets;
    std::vector<uint64_t> cbase((size_t)nt);
    std::vector<uint32_t> cnb((size_t)nt);
    uint64_t NB = 0;
    for (int32_t t = 0; t < nt; t++) {
        const uint64_t nb = (((uint64_t)std::max<int64_t>(vtop[(size_t)t], 0) + 65536u) >> BKS) + 2u;
        cbase[(size_t)t] = NB;
        cnb[(size_t)t] = (uint32_t)nb;
        NB += nb;
    }
    if (nt == 0 || NB >= 0xffffffffull) return SVT_OK;
    svt_status s;
    if ((s = upload(c, k.d_base, cbase.data(), cbase.size()))) return s;
    if ((s = upload(c, k.d_nb, cnb.data(), cnb.size()))) return s;
    if ((s = upload<uint32_t>(c, k.d_maxd, nullptr, 0, (size_t)nt))) return s;
    const uint64_t S1 = NB + 1;   // the tables' stride per array
    if ((s = upload<uint32_t>(c, k.d_off, nullptr, 0, BA_N * S1))) return s;   // (zeroed: the counts)
    if ((s = upload<uint32_t>(c, k.d_cur, nullptr, 0, BA_N * S1))) return s;
    if ((s = upload<uint32_t>(c, k.d_cap, nullptr, 0, (BA_N * S1 + 3) / 4 * 4))) return s;   // (whole uint4s: bk_zero_kernel)
    if ((s = upload<int32_t>(c, k.d_pm, nullptr, 0, 3 * S1))) return s;
    HIP_TRY(c, hipMemset(k.d_pm, 0xff, 3 * S1 * sizeof(int32_t)));   // -1: no key
    k.n = NB;
    if ((s = bk_pass(c, nullptr, true, false)) || (s = bk_check_err(c))) return s;
    // the extents: every array's buckets in order, the arrays one after the other in d_ev
    std::vector<uint32_t> cnt((size_t)(BA_N * S1));
    std::vector<int32_t> pm((size_t)(3 * S1));
    HIP_TRY(c, hipMemcpy(cnt.data(), k.d_off, cnt.size() * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(pm.data(), k.d_pm, pm.size() * 4, hipMemcpyDeviceToHost));
    uint64_t acc = 0;
    for (int A = 0; A < BA_N; A++) {
        const uint64_t a0 = acc;
        uint32_t *o = cnt.data() + (size_t)A * S1;
        for (uint64_t g = 0; g < NB; g++) {
            const uint32_t x = o[(size_t)g];
            o[(size_t)g] = (uint32_t)acc;
            acc += x;
            if (acc >= 0xffffffffull) return SVT_OK;   // (bk.ready stays false: the span lists alone)
        }
        o[(size_t)NB] = (uint32_t)acc;
        k.events[A] = acc - a0;
        if (A < 3)   // the BELOW keys' prefix maxima, within each contig
            for (int32_t t = 0; t < nt; t++) {
                int32_t m = -1;
                int32_t *q = pm.data() + (size_t)A * S1;
                for (uint64_t g = cbase[(size_t)t], g1 = g + cnb[(size_t)t]; g < g1; g++) m = q[(size_t)g] = std::max(m, q[(size_t)g]);
            }
    }
    HIP_TRY(c, hipMemcpy(k.d_off, cnt.data(), cnt.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(k.d_pm, pm.data(), pm.size() * 4, hipMemcpyHostToDevice));
    if ((s = upload<uint4>(c, k.d_ev, nullptr, 0, std::max<uint64_t>(acc, 1)))) return s;
    k.nev = (uint32_t)acc;
    k.builds = 0;   // the cursors are zero: the first filing pass is epoch 0
    if ((s = bk_pass(c, nullptr, false, false)) || (s = bk_check_err(c))) return s;
    k.builds = 1;
    k.ready = true;
    return SVT_OK;
}

// ---- the load: load_core's three steps (the host pass is loadprep::prep)

// The uploads of what the host pass made, and the allocations of the span-list build.  The CIGAR
// stream comes from host memory (stream_h), or is already on the device with STREAM_PAD zero words
// after its end (stream_d: moved from, so the context owns it from here on and frees it with the pileup).
svt_status load_upload(svt_ctx *c, const loadprep::Reads &in, const loadprep::Prep &pp, const uint32_t *stream_h,
                       DevBuf<uint32_t> *stream_d, uint64_t nops) {
    ReadCols &rc = c->reads;
    SpanIndex &x = c->ix;
    const int32_t nt = in.nt;
    const int64_t nr = (int64_t)pp.emax.size();
    const uint64_t nstream = nr > 0 ? in.soff[nr] : 0;
    if (stream_d) rc.d_cigar = std::move(*stream_d);
    x.n_ranges = pp.n_ranges;
    x.n_groups = pp.n_groups;
    svt_status s;
    if ((s = upload(c, rc.d_pos, in.pos, (size_t)nr))) return s;
    if ((s = upload(c, rc.d_emax, pp.emax.data(), (size_t)nr))) return s;
    if ((s = upload(c, rc.d_rec, reinterpret_cast<const uint4 *>(pp.rec.data()), (size_t)nr))) return s;
    if ((s = upload(c, rc.d_clip8, pp.clip8.data(), pp.clip8.size()))) return s;
    if ((s = upload(c, rc.d_off64, in.soff, nr > 0 ? (size_t)nr + 1 : 0, nr > 0 ? 0 : 1))) return s;
    if ((s = upload(c, rc.d_bkt, reinterpret_cast<const uint2 *>(pp.bkt.data()), pp.bkt.size()))) return s;
    if ((s = upload(c, rc.d_bkt_off, pp.bkt_off.data(), pp.bkt_off.size()))) return s;
    if (nt > 0) { if ((s = upload(c, rc.d_tid_off, in.tid_off, (size_t)nt + 1))) return s; }
    else if ((s = upload<int64_t>(c, rc.d_tid_off, nullptr, 0, 1))) return s;
    if (stream_d) c->dev_bytes += (nstream + STREAM_PAD) * 4u;
    else if ((s = upload(c, rc.d_cigar, stream_h, (size_t)nstream, STREAM_PAD))) return s;
    if ((s = upload(c, x.d_part, pp.part.data(), pp.part.size()))) return s;
    const size_t S = (size_t)nr + 1;
    if ((s = upload<uint64_t>(c, x.d_spoffD, nullptr, 0, S))) return s;
    if ((s = upload<uint64_t>(c, x.d_spoffI, nullptr, 0, S))) return s;
    if ((s = upload<uint2>(c, x.d_cnt, nullptr, 0, std::max<size_t>((size_t)nr, 1)))) return s;
    const size_t NR = std::max<size_t>({(size_t)x.n_ranges, (size_t)x.n_groups, (size_t)1});
    if ((s = upload<IxTot>(c, x.d_agg, nullptr, 0, NR))) return s;
    const size_t NB = (NR + IX_BLK - 1) / IX_BLK;
    if ((s = upload<IxTot>(c, x.d_bsum, nullptr, 0, NB))) return s;   // (zeroed: the first build adds into them)
    if ((s = upload<IxTot>(c, x.d_bpre, nullptr, 0, NB))) return s;
    HIP_TRY(c, hipMemset(x.d_bsum, 0, NB * sizeof(IxTot)));
    x.n_bsum = NB;
    x.bsum_dirty = false;
    if ((s = upload<uint64_t>(c, x.d_tot, nullptr, 0, IX_NTOT))) return s;
    if (!index_lane(c, nops, (uint64_t)nr)) {   // the stream walk's scratch slots
        const size_t RR = std::max<size_t>(x.n_ranges, 1);
        if ((s = upload<uint4>(c, x.d_scr, nullptr, 0, RR * IX_SCAP))) return s;
        if ((s = upload<uint2>(c, x.d_scrh, nullptr, 0, RR * IX_RCAP))) return s;
        if ((s = upload<uint32_t>(c, x.d_ovf, nullptr, 0, RR))) return s;
    }
    c->n_targets = nt;
    c->n_reads = nr;
    c->n_ops = nops;
    return SVT_OK;
}

// The first build of both indexes on the uploaded pileup, and the load's statistics.
svt_status load_build(svt_ctx *c, const std::vector<int64_t> &vtop, uint64_t nstream) {
    const SpanIndex &x = c->ix;
    svt_load_stats &ls = c->load_stats;
    svt_status s;
    if (c->n_reads > 0) {
        double ims = 0;
        if ((s = build_index(c, nullptr, true, &ims))) return s;
        ls.index_ms = ims;
        const uint64_t R = (uint64_t)c->n_reads;
        ls.span_events = x.n_evD + x.n_evI;
        ls.lead_blocks = 0;   // (no lead chunks since 0.17: refine_end's stops vote as e + 2)
        ls.slow_reads = 0;    // (no slow reads since 0.17: walks saturate at 2^30)
        // lane per read: census stream + soff + rec (24 B/read), cnt written (8 B/read); emit cnt
        // + soff + rec (32 B/read) + stream, the per-read offsets (16 B/read) written; the events
        // written.  Stream walk (one pass): stream + soff + rec (24 B/read); the staged offsets
        // (8 B/read) and events written to scratch, read back, written to their places (16 B/read
        // of offsets, 3 x 16 B/event).
        if (ls.index_kind == 1)
            ls.index_bytes = 8ull * nstream + 65ull * R + 16ull * (x.n_evD + x.n_evI);
        else
            ls.index_bytes = 4ull * nstream + 56ull * R + 48ull * (x.n_evD + x.n_evI);
        if (c->bk_on) {   // the value buckets, filed from the stream (short reads) or the span lists
            if ((s = bk_load(c, vtop))) return s;
            if (c->bk.ready) {
                uint64_t placed = 0;
                for (int A = 0; A < BA_N; A++) placed += c->bk.events[A];
                ls.bucket_index = 1;
                ls.buckets = c->bk.n;
                ls.bucket_events = placed;
                ls.bucket_bytes = ls.index_kind == 1
                    ? 4ull * nstream + 24ull * R + 28ull * placed
                    : 4ull * nstream + 32ull * R + 32ull * (x.n_evD + x.n_evI) + 28ull * placed;
            }
        }
    } else {
        for (auto *pp : {&c->ix.d_spD, &c->ix.d_spI})
            if ((s = upload<uint4>(c, *pp, nullptr, 0, 1))) return s;
    }
    HIP_TRY(c, hipDeviceSynchronize());
    uint32_t ixerr = 0;
    if ((s = take_ix_status(c, &ixerr))) return s;
    if (ixerr) return fail(c, SVT_EDEVICE, "%s", "device index build: emit overran the census's sizes");
    c->loaded = true;
    return SVT_OK;
}

// The pileup of a context from per-read columns in host memory (loadprep::Reads) and the CIGAR
// stream, in host memory or on the device (load_upload): the host pass, the uploads, the first
// build.  Called inside load_frame; t_pre_ms is what the caller spent on the columns before,
// counted into host_ms.
svt_status load_core(svt_ctx *c, const loadprep::Reads &in, const uint32_t *stream_h, DevBuf<uint32_t> *stream_d,
                     uint64_t nops, double t_pre_ms) {
    const LoadClock::time_point t_start = LoadClock::now();
    loadprep::Prep pp;
    if (const char *bad = loadprep::prep(load_limits(c), in, pp)) return fail(c, SVT_EINVAL, "pileup: %s", bad);
    c->load_stats.host_ms = t_pre_ms + ms_since(t_start);
    const LoadClock::time_point t_up = LoadClock::now();
    if (svt_status s = load_upload(c, in, pp, stream_h, stream_d, nops)) return s;
    c->load_stats.upload_ms = ms_since(t_up);
    return load_build(c, pp.vtop, c->n_reads > 0 ? in.soff[c->n_reads] : 0);
}

// What every load shares: on the context's device, the old pileup and its statistics gone first,
// body(t0) timed into total_ms.
template <typename F>
svt_status load_frame(svt_ctx *c, F body) {
    DEV_GUARD(c);
    free_pileup(c);
    c->load_stats = svt_load_stats{};
    const LoadClock::time_point t0 = LoadClock::now();
    const svt_status s = body(t0);
    c->load_stats.total_ms = ms_since(t0);
    return s;
}

svt_status load_1(svt_ctx *c, const svt_pileup_view *p) {
    if (!c || !p) return SVT_EINVAL;
    if (p->n_targets < 0 || (p->n_targets > 0 && !p->tid_off))
        return fail(c, SVT_EINVAL, "pileup: %s", "bad n_targets / tid_off");
    return load_frame(c, [&](LoadClock::time_point t0) {
        loadprep::Stream sp;
        const loadprep::View v{p->n_targets, p->tid_off, p->pos, p->endpos, p->cig_off, p->cigar, p->clip};
        if (const char *bad = loadprep::stream_prep(load_limits(c), v, sp)) return fail(c, SVT_EINVAL, "pileup: %s", bad);
        const loadprep::Reads in{p->n_targets, p->tid_off, p->pos, p->endpos, sp.nc.data(), sp.soff};
        return load_core(c, in, sp.words, nullptr, sp.nops, ms_since(t0));
    });
}

}  // namespace
}  // extern "C++"

svt_status svt_load_pileup(svt_ctx *c, const svt_pileup_view *p) {
    if (!c || !p) return SVT_EINVAL;
    if (c->subs.empty()) return load_1(c, p);
    // every device gets the whole pileup (n = device count: one "item" per device)
    const size_t D = 1 + c->subs.size();
    return for_devices(c, D, [&](svt_ctx *x, size_t lo, size_t hi) { return lo < hi ? load_1(x, p) : SVT_OK; });
}

// The value buckets rebuilt from the loaded pileup; the read columns and the span lists stay as built
// at load (without the buckets -- SVTREK_INDEX=lists, or a pileup too large for them -- the span lists
// are rebuilt instead).
svt_status svt_reindex(svt_ctx *c, void *stream) {
    if (!c) return SVT_EINVAL;
    if (!c->loaded) return fail(c, SVT_ESTATE, "%s", "svt_load_pileup not called");
    DEV_GUARD(c);
    if (c->n_reads == 0) return SVT_OK;
    const hipStream_t st = (hipStream_t)stream;
    svt_status s = order_on(c, st);   // after every launch already issued (they read the index)
    if (s) return s;
    if (!c->bk.ready) return build_index(c, st, false, nullptr);
    // the value buckets: short reads filed straight from the CIGAR stream (ixb_lane_kernel); long
    // reads walked by index_kernel and filed from its stage (ixb_copy_kernel).  A captured build files
    // through its own cursors (zeroed by the graph), a direct one through the epoch cursors
    // (svt_bucket_build.inc).
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (st) HIP_TRY(c, hipStreamIsCapturing(st, &cap));
    const bool captured = cap == hipStreamCaptureStatusActive;
    if (!index_lane(c, c->n_ops, (uint64_t)c->n_reads)) {   // long reads: the stream walk stages the events
        const IxArgs a = ix_args(c);
        hipLaunchKernelGGL(index_kernel, dim3((unsigned)((c->ix.n_ranges + IX_WPB - 1) / IX_WPB)), dim3(64 * IX_WPB), 0, st, a);
        HIP_TRY(c, hipGetLastError());
        c->ix.bsum_dirty = true;   // (its block sums are not scanned: the next span-list build clears them)
    }
    if (captured)
    {   // (the buffer is allocated in whole uint4s: upload's size below rounds it up)
        const uint64_t n4 = (BA_N * (c->bk.n + 1) + 3) / 4;
        hipLaunchKernelGGL(bk_zero_kernel, dim3((unsigned)std::min<uint64_t>((n4 + 255) / 256, 4096)), dim3(256), 0, st,
                           reinterpret_cast<uint4 *>(c->bk.d_cap.get()), n4);
        HIP_TRY(c, hipGetLastError());
    }
    if ((s = bk_pass(c, st, false, captured))) return s;
    if (!captured) c->bk.builds++;
    return SVT_OK;
}

svt_status svt_last_load_stats(const svt_ctx *c, svt_load_stats *out) {
    if (!c || !out) return SVT_EINVAL;
    *out = c->load_stats;
    return SVT_OK;
}
