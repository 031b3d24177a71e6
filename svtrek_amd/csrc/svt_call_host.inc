// svt_call_host.inc -- include/svtrek_call.h's entry points (included by svt_engine.hip inside its
// extern "C" block; the kernels are svt_call.inc).

extern "C++" {
namespace {

// p grown to n elements when cap (its present size) is smaller; call_alloc: a buffer without one.
template <typename T>
svt_status call_grow(svt_ctx *c, T *&p, uint64_t &cap, uint64_t n) {
    if (n <= cap) return SVT_OK;
    hfree(p);
    cap = 0;
    if (hipMalloc(&p, n * sizeof(T)) != hipSuccess) {
        p = nullptr;
        return fail(c, SVT_ENOMEM, "%s", "svt_call_scan: device scratch");
    }
    cap = n;
    return SVT_OK;
}

template <typename T>
svt_status call_alloc(svt_ctx *c, T *&p, uint64_t n) {
    uint64_t cap = 0;
    return call_grow(c, p, cap, n);
}

// The first scan of a loaded pileup: the segments (the buckets' extents are those of the load for
// every rebuild) and the scratch that depends on the event counts alone.
svt_status call_prepare(svt_ctx *c) {
    CallScratch &k = c->call;
    if (k.ready) return SVT_OK;
    const uint64_t nb2 = 2 * c->bk_n, N = c->bk_events[BA_S] + c->bk_events[BA_I];
    svt_status s;
    uint8_t *d_flag = nullptr;
    if ((s = call_alloc(c, d_flag, nb2))) return s;
    if ((s = call_alloc(c, k.d_seg, nb2)) || (s = call_alloc(c, k.d_ctr, 8))) {
        hfree(d_flag);
        return s;
    }
    BkIndex B = make_args(c, nullptr, nullptr, 0, false).bk;
    hipLaunchKernelGGL(call_flag_kernel, dim3((unsigned)((nb2 + 255) / 256)), dim3(256), 0, nullptr, B, c->n_targets, d_flag);
    size_t tb = 0;
    hipcub::CountingInputIterator<uint64_t> it(0);
    uint64_t *d_n = reinterpret_cast<uint64_t *>(k.d_ctr);
    hipError_t e = hipcub::DeviceSelect::Flagged(nullptr, tb, it, d_flag, k.d_seg, d_n, (int)nb2, nullptr);
    if (e == hipSuccess && (s = call_grow(c, k.d_tmp, k.tmp_cap, tb)) == SVT_OK) {
        e = hipcub::DeviceSelect::Flagged(k.d_tmp, tb, it, d_flag, k.d_seg, d_n, (int)nb2, nullptr);
        if (e == hipSuccess) e = hipMemcpy(&k.n_seg, d_n, 8, hipMemcpyDeviceToHost);
    }
    hfree(d_flag);
    if (s) return s;
    HIP_TRY(c, e);
    if ((s = call_alloc(c, k.d_keys, std::max<uint64_t>(N, 1))) || (s = call_alloc(c, k.d_cid, std::max<uint64_t>(N, 1))) ||
        (s = call_alloc(c, k.d_tmax, k.n_seg)) || (s = call_alloc(c, k.d_tprev, k.n_seg)))
        return s;
    size_t t1 = 0, t2 = 0;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveScan(nullptr, t1, k.d_tmax, k.d_tprev, hipcub::Max(), 0ull, (int)k.n_seg, nullptr));
    HIP_TRY(c, hipcub::DeviceScan::InclusiveSum(nullptr, t2, k.d_cid, k.d_cid, (int)std::max<uint64_t>(N, 1), nullptr));
    if ((s = call_grow(c, k.d_tmp, k.tmp_cap, std::max(t1, t2)))) return s;
    k.ready = true;
    return SVT_OK;
}

svt_status call_scan_1(svt_ctx *c, const svt_call_params *p, uint64_t *n_calls) {
    CallScratch &k = c->call;
    k.n_calls = 0;
    k.stats = svt_call_stats{};
    const uint64_t N = c->bk_events[BA_S] + c->bk_events[BA_I];
    if (c->n_reads == 0 || N == 0) {
        *n_calls = 0;
        return SVT_OK;
    }
    svt_status s = order_on(c, nullptr);   // after every launch already issued (svt_reindex rebuilds the buckets)
    if (s) return s;
    struct Ev {   // (destroys what was created, whichever step fails)
        hipEvent_t a = nullptr, b = nullptr;
        ~Ev() {
            if (a) (void)hipEventDestroy(a);
            if (b) (void)hipEventDestroy(b);
        }
    } evg;
    hipEvent_t &e0 = evg.a, &e1 = evg.b;
    HIP_TRY(c, hipEventCreate(&e0));
    HIP_TRY(c, hipEventCreate(&e1));
    HIP_TRY(c, hipEventRecord(e0, nullptr));
    if ((s = call_prepare(c))) return s;
    const KArgs ka = make_args(c, nullptr, nullptr, 0, false);
    CallArgs a{};
    a.bk = ka.bk;
    a.pile = ka.pile;
    a.nt = c->n_targets;
    a.n_s = (uint32_t)c->bk_events[BA_S];
    a.n_seg = k.n_seg;
    a.seg = k.d_seg;
    a.keys = k.d_keys;
    a.cid = k.d_cid;
    a.tmax = k.d_tmax;
    a.tprev = k.d_tprev;
    a.pick_n = k.d_ctr;
    a.stats = reinterpret_cast<unsigned long long *>(k.d_ctr + 2);
    a.link = (uint32_t)p->link;
    a.min_support = (uint32_t)p->min_support;
    a.types = p->types;
    const dim3 sg((unsigned)k.n_seg), sb(CALL_T);
    HIP_TRY(c, hipMemsetAsync(k.d_ctr, 0, 8 * sizeof(uint32_t), nullptr));
    hipLaunchKernelGGL(call_sort_kernel, sg, sb, 0, nullptr, a);
    size_t tb = k.tmp_cap;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveScan(k.d_tmp, tb, k.d_tmax, k.d_tprev, hipcub::Max(), 0ull, (int)k.n_seg, nullptr));
    hipLaunchKernelGGL(call_head_kernel, sg, sb, 0, nullptr, a);
    tb = k.tmp_cap;
    HIP_TRY(c, hipcub::DeviceScan::InclusiveSum(k.d_tmp, tb, k.d_cid, k.d_cid, (int)N, nullptr));
    HIP_TRY(c, hipGetLastError());
    uint32_t ncl = 0, ncl_s = 0;   // clusters; those of array S (the DEL clusters come first)
    HIP_TRY(c, hipMemcpy(&ncl, k.d_cid + (N - 1), 4, hipMemcpyDeviceToHost));
    if (a.n_s) HIP_TRY(c, hipMemcpy(&ncl_s, k.d_cid + (a.n_s - 1), 4, hipMemcpyDeviceToHost));
    uint32_t picked[2] = {0, 0};   // calls, the DEL calls among them
    if (ncl) {
        size_t need = 0;
        hipcub::CountingInputIterator<uint32_t> it(0);
        HIP_TRY(c, hipcub::DeviceSelect::Flagged(nullptr, need, it, k.d_flag, k.d_pick, k.d_ctr, (int)ncl, nullptr));
        if ((s = call_grow(c, k.d_acc, k.acc_cap, ncl)) || (s = call_grow(c, k.d_pick, k.pick_cap, ncl)) ||
            (s = call_grow(c, k.d_flag, k.flag_cap, ncl)) || (s = call_grow(c, k.d_tmp, k.tmp_cap, need)))
            return s;
        a.acc = k.d_acc;
        a.pick = k.d_pick;
        HIP_TRY(c, hipMemsetAsync(k.d_acc, 0, (size_t)ncl * sizeof(CallAcc), nullptr));
        hipLaunchKernelGGL(call_accum_kernel, sg, sb, 0, nullptr, a);
        hipLaunchKernelGGL(call_pick_kernel, dim3((ncl + 255u) / 256u), dim3(256), 0, nullptr, a, ncl, ncl_s, k.d_flag,
                           k.d_ctr + 1);
        tb = k.tmp_cap;
        HIP_TRY(c, hipcub::DeviceSelect::Flagged(k.d_tmp, tb, it, k.d_flag, k.d_pick, k.d_ctr, (int)ncl, nullptr));
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpy(picked, k.d_ctr, sizeof picked, hipMemcpyDeviceToHost));
    }
    const uint32_t npick = picked[0], ndel = std::min(picked[1], picked[0]);
    if (npick) {
        if ((s = call_grow(c, k.d_calls, k.calls_cap, npick)) || (s = call_grow(c, k.d_raw, k.raw_cap, npick))) return s;
        hipLaunchKernelGGL(call_emit_kernel, dim3((npick + WPB - 1) / WPB), dim3(64 * WPB), 0, nullptr, a, npick, k.d_raw);
        hipLaunchKernelGGL(call_merge_kernel, dim3((npick + 255u) / 256u), dim3(256), 0, nullptr, k.d_raw, npick, ndel,
                           k.d_calls);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipEventRecord(e1, nullptr));
    HIP_TRY(c, hipEventSynchronize(e1));
    unsigned long long st[3] = {};
    HIP_TRY(c, hipMemcpy(st, k.d_ctr + 2, sizeof st, hipMemcpyDeviceToHost));
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, e0, e1));
    k.stats.events = st[0];
    k.stats.skipped = st[1];
    k.stats.big_buckets = st[2];
    k.stats.clusters = ncl;
    k.stats.calls = npick;
    k.stats.scan_ms = ms;
    k.n_calls = npick;
    *n_calls = npick;
    return SVT_OK;
}

}  // namespace
}  // extern "C++"

void svt_call_default_params(const svt_ctx *c, svt_call_params *out) {
    if (!out) return;
    out->link = 10;
    out->min_support = c ? std::max(c->prm.consensus_min_count, 1) : 3;
    out->types = (1u << SVT_INS) | (1u << SVT_DEL);
    out->pad = 0;
}

svt_status svt_call_scan(svt_ctx *c, const svt_call_params *p, uint64_t *n_calls) {
    if (!c) return SVT_EINVAL;
    if (!p || !n_calls) return fail(c, SVT_EINVAL, "%s", "null params/n_calls");
    if (p->link < 0 || p->link > (1 << 20) || p->min_support < 1 || !(p->types & ((1u << SVT_INS) | (1u << SVT_DEL))))
        return fail(c, SVT_EINVAL, "%s", "svt_call_scan: link in [0, 2^20], min_support >= 1 and a type bit of DEL / INS");
    if (!c->loaded) return fail(c, SVT_ESTATE, "%s", "svt_load_pileup not called");
    if (c->n_reads != 0 && !c->bk_ready)
        return fail(c, SVT_ESTATE, "%s",
                    "svt_call_scan needs the value buckets (not built: SVTREK_INDEX=lists, or a pileup past 2^32 events)");
    if (c->bk_nev >= 0x7fffffffu || 2 * c->bk_n >= 0x7fffffffull)   // (the scans' and the sort network's 32-bit counts)
        return fail(c, SVT_ESTATE, "%s", "svt_call_scan: 2^31 events or buckets and more are not supported");
    DEV_GUARD(c);
    return call_scan_1(c, p, n_calls);
}

svt_status svt_call_fetch(svt_ctx *c, uint64_t first, uint64_t n, svt_call *out) {
    if (!c) return SVT_EINVAL;
    if (first > c->call.n_calls || n > c->call.n_calls - first) return fail(c, SVT_EINVAL, "%s", "svt_call_fetch: range past the scanned calls");
    if (n == 0) return SVT_OK;
    if (!out) return fail(c, SVT_EINVAL, "%s", "null out");
    DEV_GUARD(c);
    HIP_TRY(c, hipMemcpy(out, c->call.d_calls + first, n * sizeof(svt_call), hipMemcpyDeviceToHost));
    return SVT_OK;
}

svt_status svt_call_device(svt_ctx *c, const svt_call **d_calls, uint64_t *n) {
    if (!c) return SVT_EINVAL;
    if (!d_calls || !n) return fail(c, SVT_EINVAL, "%s", "null d_calls/n");
    *d_calls = c->call.n_calls ? c->call.d_calls : nullptr;
    *n = c->call.n_calls;
    return SVT_OK;
}

svt_status svt_call_stats_get(const svt_ctx *c, svt_call_stats *out) {
    if (!c || !out) return SVT_EINVAL;
    *out = c->call.stats;
    return SVT_OK;
}
