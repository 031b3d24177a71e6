// svt_call_host.inc -- include/svtrek_call.h's entry points (included by svt_engine.hip inside its
// extern "C" block; the kernels are svt_call.inc).

extern "C++" {
namespace {

constexpr const char *CALL_MEM = "svt_call_scan: device scratch";

// A pass's counters as they lie in k.d_ctr: zeroed when the pass begins, read back once at its end.
struct CallCtr {
    uint32_t picked, picked_del;                       // calls, the DEL calls among them
    unsigned long long events, skipped, big_buckets;   // call_sort_kernel's
    unsigned long long split, groups, split_big;       // call_split_kernel's (len_permille > 0)
    uint32_t candidates, pad;                          // call_split_1's select
};
constexpr size_t CALL_NCTR = sizeof(CallCtr) / sizeof(uint32_t);
static_assert(sizeof(CallCtr) == 64 && offsetof(CallCtr, events) == 8 && offsetof(CallCtr, split) == 32, "addressed by word");

// The index a scan runs on: the value buckets, or a derived index in their shape (CallIndex) -- the
// merged index (merge_gap > 0), the union of either with the junction events (junctions = 1), the
// rearrangement index (the second pass of rearr != 0).  The segments depend on the extents, so each has
// its own; the rest of the scratch is shared and only ever grown.
struct CallView {
    BkIndex bk;
    uint64_t n_s, n_i;            // events of arrays S and I
    CallSegs *segs;
};
CallView plain_view(svt_ctx *c) {
    return CallView{c->bk.view(), c->bk.events[BA_S], c->bk.events[BA_I], &c->call.segs};
}
CallView index_view(svt_ctx *c, CallIndex &ix) {
    CallView v{plain_view(c).bk, ix.events[0], ix.events[1], &ix.segs};
    v.bk.ev = ix.d_ev;
    v.bk.off = ix.d_off;
    v.bk.pm = nullptr;            // (the refine side's: no kernel of the scan or the genotypes reads it)
    return v;
}
// (the union is built on the merged index where both are asked for: svt_junction_host.inc)
CallView call_view(svt_ctx *c, bool merged, bool junction) {
    return junction ? index_view(c, c->call.jn) : merged ? index_view(c, c->call.mg) : plain_view(c);
}

svt_status junction_build(svt_ctx *c, uint32_t gap, uint32_t min_len);   // svt_junction_host.inc
svt_status rearr_build(svt_ctx *c);                                      // svt_rearr_host.inc
svt_status bnd_build(svt_ctx *c);                                        // svt_bnd_host.inc
svt_status bnd_stage(svt_ctx *c, const svt_call_params *p, const svt_call *others, uint32_t n_other, uint64_t *total);

// The first scan of a loaded pileup (of a merged index): the segments (the buckets' extents are those
// of the load for every rebuild) and the scratch that depends on the event counts alone.
svt_status call_prepare(svt_ctx *c, const CallView &v) {
    CallScratch &k = c->call;
    if (v.segs->ready) return SVT_OK;
    const uint64_t nb2 = 2 * c->bk.n, N = v.n_s + v.n_i;
    svt_status s;
    DevBuf<uint8_t> d_flag;
    DevBuf<uint64_t> &d_seg = v.segs->d_seg;
    uint64_t &n_seg = v.segs->n_seg;
    if ((s = nomem(c, d_flag.reserve(nb2), CALL_MEM)) || (s = nomem(c, d_seg.reserve(nb2), CALL_MEM)) ||
        (s = nomem(c, k.d_ctr.reserve(CALL_NCTR), CALL_MEM)))
        return s;
    const BkIndex &B = v.bk;
    hipLaunchKernelGGL(call_flag_kernel, dim3((unsigned)((nb2 + 255) / 256)), dim3(256), 0, nullptr, B, c->n_targets, d_flag);
    size_t tb = 0;
    hipcub::CountingInputIterator<uint64_t> it(0);
    uint64_t *d_n = reinterpret_cast<uint64_t *>(k.d_ctr.get());
    HIP_TRY(c, hipcub::DeviceSelect::Flagged(nullptr, tb, it, d_flag.get(), d_seg.get(), d_n, (int)nb2, nullptr));
    if ((s = nomem(c, k.d_tmp.reserve(tb), CALL_MEM))) return s;
    HIP_TRY(c, hipcub::DeviceSelect::Flagged(k.d_tmp.get(), tb, it, d_flag.get(), d_seg.get(), d_n, (int)nb2, nullptr));
    HIP_TRY(c, hipMemcpy(&n_seg, d_n, 8, hipMemcpyDeviceToHost));
    d_flag.reset();
    if ((s = nomem(c, k.d_keys.reserve(std::max<uint64_t>(N, 1)), CALL_MEM)) ||
        (s = nomem(c, k.d_cid.reserve(std::max<uint64_t>(N, 1)), CALL_MEM)) ||
        (s = nomem(c, k.d_tmax.reserve(n_seg), CALL_MEM)) || (s = nomem(c, k.d_tprev.reserve(n_seg), CALL_MEM)))
        return s;
    size_t t1 = 0, t2 = 0;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveScan(nullptr, t1, k.d_tmax.get(), k.d_tprev.get(), hipcub::Max(), 0ull,
                                                 (int)n_seg, nullptr));
    HIP_TRY(c, hipcub::DeviceScan::InclusiveSum(nullptr, t2, k.d_cid.get(), k.d_cid.get(), (int)std::max<uint64_t>(N, 1), nullptr));
    if ((s = nomem(c, k.d_tmp.reserve(std::max(t1, t2)), CALL_MEM))) return s;
    v.segs->ready = true;
    return SVT_OK;
}

// The split by length of a scan with len_permille > 0 (svt_call.inc), after call_accum_kernel: the
// units' records into k.d_uacc in the order the calls take, their number and that of array S's into
// *nu / *nu_s.  Its scratch is allocated here, by the first such scan, and freed with the pileup.
svt_status call_split_1(svt_ctx *c, const CallArgs &a, uint32_t n_keys, uint32_t ncl, uint32_t ncl_s, uint32_t *nu, uint32_t *nu_s) {
    CallScratch &k = c->call;
    svt_status s;
    if ((s = nomem(c, k.d_cflag.reserve(ncl), CALL_MEM)) || (s = nomem(c, k.d_cand.reserve(ncl), CALL_MEM)) ||
        (s = nomem(c, k.d_kend.reserve(ncl), CALL_MEM)) || (s = nomem(c, k.d_unit.reserve(ncl), CALL_MEM)))
        return s;
    uint32_t *d_ncand = k.d_ctr + offsetof(CallCtr, candidates) / 4;
    hipcub::CountingInputIterator<uint32_t> it(0);
    size_t t1 = 0, t2 = 0;
    HIP_TRY(c, hipcub::DeviceSelect::Flagged(nullptr, t1, it, k.d_cflag.get(), k.d_cand.get(), d_ncand, (int)ncl, nullptr));
    HIP_TRY(c, hipcub::DeviceScan::InclusiveSum(nullptr, t2, k.d_kend.get(), k.d_kend.get(), (int)ncl, nullptr));
    if ((s = nomem(c, k.d_tmp.reserve(std::max(t1, t2)), CALL_MEM))) return s;
    const dim3 cg((ncl + 255u) / 256u), cb(256);
    hipLaunchKernelGGL(call_cand_kernel, cg, cb, 0, nullptr, a, ncl, k.d_cflag, k.d_kend, k.d_unit);
    size_t tb = k.d_tmp.cap();
    HIP_TRY(c, hipcub::DeviceSelect::Flagged(k.d_tmp.get(), tb, it, k.d_cflag.get(), k.d_cand.get(), d_ncand, (int)ncl, nullptr));
    tb = k.d_tmp.cap();
    HIP_TRY(c, hipcub::DeviceScan::InclusiveSum(k.d_tmp.get(), tb, k.d_kend.get(), k.d_kend.get(), (int)ncl, nullptr));
    HIP_TRY(c, hipGetLastError());
    uint32_t ncand = 0, nkeys = 0;   // candidates; their items (at most the events: 32 bits hold them)
    HIP_TRY(c, hipMemcpy(&ncand, d_ncand, 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(&nkeys, k.d_kend + (ncl - 1), 4, hipMemcpyDeviceToHost));
    CallSplit sp{};
    sp.cflag = k.d_cflag;
    sp.cand = k.d_cand;
    sp.kend = k.d_kend;
    sp.unit = k.d_unit;
    sp.stats = reinterpret_cast<unsigned long long *>(k.d_ctr + offsetof(CallCtr, split) / 4);
    sp.n_keys = n_keys;
    const dim3 sg(ncand), sb(CALL_T);
    if (ncand) {
        if ((s = nomem(c, k.d_skeys.reserve(nkeys), CALL_MEM))) return s;
        sp.skeys = k.d_skeys;
        hipLaunchKernelGGL(call_split_kernel, sg, sb, 0, nullptr, a, sp);
    }
    tb = k.d_tmp.cap();
    HIP_TRY(c, hipcub::DeviceScan::InclusiveSum(k.d_tmp.get(), tb, k.d_unit.get(), k.d_unit.get(), (int)ncl, nullptr));
    HIP_TRY(c, hipGetLastError());
    *nu = *nu_s = 0;
    HIP_TRY(c, hipMemcpy(nu, k.d_unit + (ncl - 1), 4, hipMemcpyDeviceToHost));
    if (ncl_s) HIP_TRY(c, hipMemcpy(nu_s, k.d_unit + (ncl_s - 1), 4, hipMemcpyDeviceToHost));
    if (*nu < ncl || *nu >= 0x7fffffffu)   // (at most one unit an item)
        return fail(c, SVT_ESTATE, "%s", "svt_call_scan: the split's unit count is out of range");
    if ((s = nomem(c, k.d_uacc.reserve(*nu), CALL_MEM))) return s;
    sp.uacc = k.d_uacc;
    if (ncand) {
        if ((s = nomem(c, k.d_gacc.reserve(*nu), CALL_MEM))) return s;
        sp.gacc = k.d_gacc;
        HIP_TRY(c, hipMemsetAsync(k.d_gacc, 0, (size_t)*nu * sizeof(CallAcc), nullptr));
        hipLaunchKernelGGL(call_group_kernel, sg, sb, 0, nullptr, a, sp);
    }
    hipLaunchKernelGGL(call_unit_kernel, cg, cb, 0, nullptr, a, sp, ncl);
    if (ncand) hipLaunchKernelGGL(call_order_kernel, sg, sb, 0, nullptr, a, sp);
    HIP_TRY(c, hipGetLastError());
    return SVT_OK;
}

// la[0 .. na) and lb[0 .. nb) merged into dst (merge_lists_kernel): the destination reserved, the launch checked.
svt_status call_merge(svt_ctx *c, const svt_call *la, uint32_t na, const svt_call *lb, uint32_t nb, DevBuf<svt_call> &dst) {
    const uint64_t n = (uint64_t)na + nb;
    if (n == 0) return SVT_OK;
    if (svt_status s = nomem(c, dst.reserve(n), CALL_MEM)) return s;
    hipLaunchKernelGGL(merge_lists_kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, nullptr, la, na, lb, nb, dst.get());
    HIP_TRY(c, hipGetLastError());
    return SVT_OK;
}

// One pass of the scan over view v: the sort, the link, the accumulation, the split by length and the pick,
// then the records -- call_emit_kernel's for the view, or for the rearrangement index (svt_rearr.inc) -- and
// the merge of the pass's two lists into dst.  What it counted comes back in *out.
struct CallPass {
    uint32_t ncl = 0, npick = 0;
    CallCtr ctr{};
};
svt_status call_pass(svt_ctx *c, const svt_call_params *p, const CallView &v, uint32_t types, bool rearr, DevBuf<svt_call> &dst,
                     CallPass *out) {
    CallScratch &k = c->call;
    const uint64_t N = v.n_s + v.n_i;
    svt_status s;
    if ((s = call_prepare(c, v))) return s;
    const uint64_t n_seg = v.segs->n_seg;
    const KArgs ka = make_args(c, nullptr, nullptr, 0, false);
    CallArgs a{};
    a.bk = v.bk;
    a.pile = ka.pile;
    a.nt = c->n_targets;
    a.n_s = (uint32_t)v.n_s;
    a.n_seg = n_seg;
    a.seg = v.segs->d_seg.get();
    a.keys = k.d_keys;
    a.cid = k.d_cid;
    a.tmax = k.d_tmax;
    a.tprev = k.d_tprev;
    a.pick_n = k.d_ctr;
    a.stats = reinterpret_cast<unsigned long long *>(k.d_ctr + 2);
    a.link = (uint32_t)p->link;
    a.min_support = (uint32_t)p->min_support;
    a.types = types;
    a.permille = p->len_permille;
    const dim3 sg((unsigned)n_seg), sb(CALL_T);
    HIP_TRY(c, hipMemsetAsync(k.d_ctr, 0, sizeof(CallCtr), nullptr));
    hipLaunchKernelGGL(call_sort_kernel, sg, sb, 0, nullptr, a);
    size_t tb = k.d_tmp.cap();
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveScan(k.d_tmp.get(), tb, k.d_tmax.get(), k.d_tprev.get(), hipcub::Max(), 0ull,
                                                 (int)n_seg, nullptr));
    hipLaunchKernelGGL(call_head_kernel, sg, sb, 0, nullptr, a);
    tb = k.d_tmp.cap();
    HIP_TRY(c, hipcub::DeviceScan::InclusiveSum(k.d_tmp.get(), tb, k.d_cid.get(), k.d_cid.get(), (int)N, nullptr));
    HIP_TRY(c, hipGetLastError());
    uint32_t ncl = 0, ncl_s = 0;   // clusters; those of array S (the DEL clusters come first)
    HIP_TRY(c, hipMemcpy(&ncl, k.d_cid + (N - 1), 4, hipMemcpyDeviceToHost));
    if (a.n_s) HIP_TRY(c, hipMemcpy(&ncl_s, k.d_cid + (a.n_s - 1), 4, hipMemcpyDeviceToHost));
    if (ncl) {
        size_t need = 0;
        hipcub::CountingInputIterator<uint32_t> it(0);
        HIP_TRY(c, hipcub::DeviceSelect::Flagged(nullptr, need, it, k.d_flag.get(), k.d_pick.get(), k.d_ctr.get(), (int)ncl, nullptr));
        if ((s = nomem(c, k.d_acc.reserve(ncl), CALL_MEM)) || (s = nomem(c, k.d_pick.reserve(ncl), CALL_MEM)) ||
            (s = nomem(c, k.d_flag.reserve(ncl), CALL_MEM)) || (s = nomem(c, k.d_tmp.reserve(need), CALL_MEM)))
            return s;
        if (a.permille && (s = nomem(c, k.d_first.reserve(ncl), CALL_MEM))) return s;
        a.acc = k.d_acc;
        a.pick = k.d_pick;
        a.first = a.permille ? k.d_first.get() : nullptr;
        HIP_TRY(c, hipMemsetAsync(k.d_acc, 0, (size_t)ncl * sizeof(CallAcc), nullptr));
        hipLaunchKernelGGL(call_accum_kernel, sg, sb, 0, nullptr, a);
        uint32_t nu = ncl, nu_s = ncl_s;   // what is picked from: the clusters, or the units of a split scan
        if (a.permille) {
            if ((s = call_split_1(c, a, (uint32_t)N, ncl, ncl_s, &nu, &nu_s))) return s;
            need = 0;
            HIP_TRY(c, hipcub::DeviceSelect::Flagged(nullptr, need, it, k.d_flag.get(), k.d_pick.get(), k.d_ctr.get(), (int)nu, nullptr));
            if ((s = nomem(c, k.d_pick.reserve(nu), CALL_MEM)) || (s = nomem(c, k.d_flag.reserve(nu), CALL_MEM)) ||
                (s = nomem(c, k.d_tmp.reserve(need), CALL_MEM)))
                return s;
            a.acc = k.d_uacc;
            a.pick = k.d_pick;
        }
        hipLaunchKernelGGL(call_pick_kernel, dim3((nu + 255u) / 256u), dim3(256), 0, nullptr, a, nu, nu_s, k.d_flag,
                           k.d_ctr + 1);
        tb = k.d_tmp.cap();
        HIP_TRY(c, hipcub::DeviceSelect::Flagged(k.d_tmp.get(), tb, it, k.d_flag.get(), k.d_pick.get(), k.d_ctr.get(), (int)nu, nullptr));
        HIP_TRY(c, hipGetLastError());
    }
    CallCtr &ctr = out->ctr;   // (behind every kernel of the pass that counts)
    HIP_TRY(c, hipMemcpy(&ctr, k.d_ctr, sizeof ctr, hipMemcpyDeviceToHost));
    const uint32_t npick = ctr.picked, ndel = std::min(ctr.picked_del, ctr.picked);
    if (npick) {
        if ((s = nomem(c, k.d_raw.reserve(npick), CALL_MEM))) return s;
        const dim3 eg((npick + WPB - 1) / WPB), eb(64 * WPB);
        if (rearr) hipLaunchKernelGGL(call_emit_kernel<true>, eg, eb, 0, nullptr, a, npick, k.d_raw);
        else hipLaunchKernelGGL(call_emit_kernel<false>, eg, eb, 0, nullptr, a, npick, k.d_raw);
        if ((s = call_merge(c, k.d_raw + ndel, npick - ndel, k.d_raw, ndel, dst))) return s;   // (la: the INS calls, behind the ndel DEL calls)
    }
    out->ncl = ncl;
    out->npick = npick;
    return SVT_OK;
}

// A pass's counts added to the scan's stats (zeroed when the scan began).
void call_pass_stats(CallScratch::Last &l, const CallPass &ps) {
    l.call_stats.events += ps.ctr.events;
    l.call_stats.skipped += ps.ctr.skipped;
    l.call_stats.big_buckets += ps.ctr.big_buckets;
    l.call_stats.clusters += ps.ncl;
    l.call_stats.calls += ps.npick;
    l.split_stats.candidates += ps.ctr.candidates;
    l.split_stats.split += ps.ctr.split;
    l.split_stats.groups += ps.ctr.groups;
    l.split_stats.big += ps.ctr.split_big;
}

svt_status call_scan_1(svt_ctx *c, const svt_call_params *p, uint64_t *n_calls) {
    CallScratch &k = c->call;
    k.n_calls = 0;
    k.scanned = true;
    k.last = CallScratch::Last{};   // (what it ran on: set once that index is built)
    const bool merged = p->merge_gap != 0u, junction = p->junctions != 0u;
    const uint32_t rearr = p->rearr, base_types = p->types & ((1u << SVT_INS) | (1u << SVT_DEL));
    *n_calls = 0;
    if (c->n_reads == 0) {   // (no index to build: every site of such a pileup is invalid)
        k.last.merged = merged;
        k.last.junction = junction;
        k.last.rearr = rearr;
        k.last.bnd = p->bnd;   // (and its table has no record)
        return SVT_OK;
    }
    svt_status s = order_on(c, nullptr);   // after every launch already issued (svt_reindex rebuilds the buckets)
    if (s) return s;
    if (merged) {   // (before the scan's clock: the build runs once per pileup and (gap, min))
        if ((s = callmerge_build(c, p->merge_gap, p->merge_min))) return s;
        k.last.merge_stats = k.mg.stats;
    }
    if (junction) {   // (likewise: once per pileup, table and base view)
        if ((s = junction_build(c, p->merge_gap, p->merge_min))) return s;
        k.last.junction_stats = k.jn.stats;
    }
    if (rearr) {   // (likewise: once per pileup and table)
        if ((s = rearr_build(c))) return s;
        k.last.rearr_stats = k.rr.stats;
    }
    if (p->bnd) {   // (likewise: once per pileup and table; svt_bnd_host.inc)
        if ((s = bnd_build(c))) return s;
        k.last.bnd_stats = k.bn.stats;
        k.last.call_stats.events += k.bn.stats.items;
        k.last.call_stats.skipped += k.bn.stats.skipped;
    }
    k.last.merged = merged;
    k.last.junction = junction;
    k.last.rearr = rearr;
    k.last.bnd = p->bnd;
    const bool bnd = p->bnd && k.bn.n_items != 0;   // the BND stage runs
    const CallView v = call_view(c, merged, junction);
    const uint64_t N = base_types ? v.n_s + v.n_i : 0;   // (no DEL / INS bit: a rearrangement- or breakend-only scan)
    if (N == 0 && !rearr && !bnd) return SVT_OK;
    DevEvent e0, e1;
    HIP_TRY(c, e0.create());
    HIP_TRY(c, e1.create());
    HIP_TRY(c, hipEventRecord(e0, nullptr));
    // Three stages, each handing its sorted list (list, total) to the next; the last one's lands in k.d_calls.
    const svt_call *list = nullptr;
    uint64_t total = 0;
    if (N) {   // the pass over the view
        DevBuf<svt_call> &dst = rearr || bnd ? k.d_list1 : k.d_calls;
        CallPass ps{};
        if ((s = call_pass(c, p, v, p->types, false, dst, &ps))) return s;
        call_pass_stats(k.last, ps);
        list = dst.get(), total = ps.npick;
    }
    if (rearr) {   // the pass over the rearrangement index (svt_rearr.inc), its list merged behind the first
        DevBuf<svt_call> &dst = bnd ? k.d_list2 : k.d_calls;
        const CallView rv = index_view(c, k.rr);
        const uint32_t rtypes = ((rearr >> SVT_DUP) & 1u) << SVT_DEL | ((rearr >> SVT_INV) & 1u) << SVT_INS;
        CallPass pr{};
        if (rv.n_s + rv.n_i != 0) {   // (no counters of a pass that does not run)
            if ((s = call_pass(c, p, rv, rtypes, true, k.rr.d_calls, &pr))) return s;
            call_pass_stats(k.last, pr);
            k.last.rearr_stats.skipped = pr.ctr.skipped;
            k.last.rearr_stats.clusters = pr.ncl;
            k.last.rearr_stats.calls = pr.npick;
        }
        if (total + pr.npick > 0x7fffffffull) return fail(c, SVT_ESTATE, "%s", "svt_call_scan: more than 2^31 - 1 calls are not supported");
        if ((s = call_merge(c, list, (uint32_t)total, k.rr.d_calls.get(), pr.npick, dst))) return s;
        list = dst.get(), total += pr.npick;
    }
    if (bnd && (s = bnd_stage(c, p, list, (uint32_t)total, &total))) return s;   // its list merged behind the others (svt_bnd_host.inc)
    HIP_TRY(c, hipEventRecord(e1, nullptr));
    HIP_TRY(c, hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, e0, e1));
    k.last.call_stats.scan_ms = ms;
    k.n_calls = total;
    *n_calls = total;
    return SVT_OK;
}

}  // namespace
}  // extern "C++"

void svt_call_default_params(const svt_ctx *c, svt_call_params *out) {
    if (!out) return;
    out->link = 10;
    out->min_support = c ? std::max(c->prm.consensus_min_count, 1) : 3;
    out->types = (1u << SVT_INS) | (1u << SVT_DEL);
    out->len_permille = 0;
    out->merge_gap = 0;
    out->merge_min = 20;
    out->junctions = 0;
    out->rearr = 0;
    out->bnd = 0;
}

svt_status svt_call_scan(svt_ctx *c, const svt_call_params *p, uint64_t *n_calls) {
    if (!c) return SVT_EINVAL;
    if (!p || !n_calls) return fail(c, SVT_EINVAL, "%s", "null params/n_calls");
    if (p->rearr & ~((1u << SVT_DUP) | (1u << SVT_INV))) return fail(c, SVT_EINVAL, "%s", "svt_call_scan: rearr is a mask of the DUP and INV bits");
    if (p->bnd > 1u) return fail(c, SVT_EINVAL, "%s", "svt_call_scan: bnd is 0 or 1");
    if (p->link < 0 || p->link > (1 << 20) || p->min_support < 1 || (!(p->types & ((1u << SVT_INS) | (1u << SVT_DEL))) && !p->rearr && !p->bnd))
        return fail(c, SVT_EINVAL, "%s", "svt_call_scan: link in [0, 2^20], min_support >= 1 and a type bit of DEL / INS");
    if (p->len_permille > 1000u) return fail(c, SVT_EINVAL, "%s", "svt_call_scan: len_permille in [0, 1000]");
    if (p->merge_gap > (1u << 20) || (p->merge_gap != 0u && (p->merge_min < 1u || p->merge_min > (uint32_t)SV_MIN_LENGTH)))
        return fail(c, SVT_EINVAL, "%s", "svt_call_scan: merge_gap in [0, 2^20] and, with it, merge_min in [1, 50]");
    if (p->junctions > 1u) return fail(c, SVT_EINVAL, "%s", "svt_call_scan: junctions is 0 or 1");
    if (!c->loaded) return fail(c, SVT_ESTATE, "%s", "svt_load_pileup not called");
    if (p->junctions && !c->call.jn.loaded)
        return fail(c, SVT_ESTATE, "%s", "svt_call_scan: junctions = 1 without svt_load_junctions for the loaded pileup");
    if (p->rearr && !c->call.jn.loaded)
        return fail(c, SVT_ESTATE, "%s", "svt_call_scan: rearr != 0 without svt_load_junctions for the loaded pileup");
    if (p->bnd && !c->call.jn.loaded)
        return fail(c, SVT_ESTATE, "%s", "svt_call_scan: bnd = 1 without svt_load_junctions for the loaded pileup");
    if (p->bnd && (int64_t)c->n_targets >= (int64_t)(1 << 30) - 1)
        return fail(c, SVT_ESTATE, "%s", "svt_call_scan: bnd = 1 with 2^30 - 1 targets or more is not supported");
    if (c->n_reads != 0 && !c->bk.ready)
        return fail(c, SVT_ESTATE, "%s",
                    "svt_call_scan needs the value buckets (not built: SVTREK_INDEX=lists, or a pileup past 2^32 events)");
    if (c->bk.nev >= 0x7fffffffu || 2 * c->bk.n >= 0x7fffffffull)   // (the scans' and the sort network's 32-bit counts)
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
    *d_calls = c->call.n_calls ? c->call.d_calls.get() : nullptr;
    *n = c->call.n_calls;
    return SVT_OK;
}

svt_status svt_call_stats_get(const svt_ctx *c, svt_call_stats *out) {
    if (!c || !out) return SVT_EINVAL;
    *out = c->call.last.call_stats;
    return SVT_OK;
}

svt_status svt_call_split_stats_get(const svt_ctx *c, svt_call_split_stats *out) {
    if (!c || !out) return SVT_EINVAL;
    *out = c->call.last.split_stats;
    return SVT_OK;
}

svt_status svt_call_merge_stats_get(const svt_ctx *c, svt_call_merge_stats *out) {
    if (!c || !out) return SVT_EINVAL;
    *out = c->call.last.merge_stats;
    return SVT_OK;
}
