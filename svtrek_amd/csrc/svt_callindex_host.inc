// svt_callindex_host.inc -- the one build path of svt_call_scan's derived indexes (included by
// svt_engine.hip inside its extern "C" block before svt_callmerge_host.inc; the device side is
// svt_callindex.inc, the owner CallIndex is svt_devmem.inc's).

extern "C++" {
namespace {

// What an index words its failures with, and the most events it may hold.
struct CallIndexText {
    const char *mem;              // nomem's label
    const char *too_many;         // the message past max_events
    const char *what;             // the prefix of "...: the counts disagree" / "...: the filing disagrees with its count"
    uint64_t max_events;
};
// What the counting pass's totals let an index expect: its events, and the bounds of array S's.
struct CallIndexExpect {
    uint64_t n, ns_min, ns_max;
};

// Index ix of the loaded pileup, dropped and built anew: count(f) launches the counting pass (and adds
// the base extents, where there are any) into f.off, the slot counters are summed into tot[], expect(tot)
// says what must come of them, an exclusive sum per row gives the extents, file(f) launches the filing
// pass.  *build_ms is the time of it all on the device.
template <int NSTAT, class Count, class Expect, class File>
svt_status callindex_build(svt_ctx *c, CallIndex &ix, const CallIndexText &t, uint64_t (&tot)[NSTAT], double *build_ms, Count count,
                           Expect expect, File file) {
    ix.drop();
    const uint64_t S1 = c->bk.n + 1;
    constexpr size_t NST = (size_t)NSTAT * BK_SLOTS;
    svt_status s;
    DevBuf<uint32_t> d_cur;
    DevBuf<unsigned long long> d_stat;   // the slot counters, then the error word
    DevBuf<uint8_t> d_tmp;
    if ((s = nomem(c, ix.d_off.reserve(BA_N * S1), t.mem)) || (s = nomem(c, d_cur.reserve(2 * S1), t.mem)) ||
        (s = nomem(c, d_stat.reserve(NST + 1), t.mem)))
        return s;
    DevEvent e0, e1;
    HIP_TRY(c, e0.create());
    HIP_TRY(c, e1.create());
    HIP_TRY(c, hipEventRecord(e0, nullptr));
    HIP_TRY(c, hipMemsetAsync(ix.d_off, 0, BA_N * S1 * sizeof(uint32_t), nullptr));
    HIP_TRY(c, hipMemsetAsync(d_cur, 0, 2 * S1 * sizeof(uint32_t), nullptr));
    HIP_TRY(c, hipMemsetAsync(d_stat, 0, (NST + 1) * sizeof(unsigned long long), nullptr));
    BkFile f{c->bk.d_base, c->bk.d_nb, c->bk.n, ix.d_off, d_cur, nullptr, 0u, d_stat, reinterpret_cast<uint32_t *>(d_stat + NST)};
    count(f);
    HIP_TRY(c, hipGetLastError());
    std::vector<unsigned long long> st(NST);
    HIP_TRY(c, hipMemcpy(st.data(), d_stat, NST * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int q = 0; q < NSTAT; q++) tot[q] = 0;
    for (uint32_t i = 0; i < BK_SLOTS; i++)
        for (int q = 0; q < NSTAT; q++) tot[q] += st[(size_t)NSTAT * i + q];
    const CallIndexExpect x = expect(tot);
    if (x.n > t.max_events) return fail(c, SVT_ESTATE, "%s", t.too_many);
    // the extents: row S from 0, row I behind it (the counts' slot nbk is zero: the row's end)
    uint32_t *offS = ix.d_off + (size_t)BA_S * S1, *offI = ix.d_off + (size_t)BA_I * S1;
    size_t tb = 0;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveScan(nullptr, tb, offS, offS, hipcub::Sum(), 0u, (int)S1, nullptr));
    if ((s = nomem(c, d_tmp.reserve(tb), t.mem))) return s;
    size_t t1 = d_tmp.cap();
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveScan(d_tmp.get(), t1, offS, offS, hipcub::Sum(), 0u, (int)S1, nullptr));
    uint32_t nS = 0;
    HIP_TRY(c, hipMemcpy(&nS, offS + c->bk.n, 4, hipMemcpyDeviceToHost));
    t1 = d_tmp.cap();
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveScan(d_tmp.get(), t1, offI, offI, hipcub::Sum(), nS, (int)S1, nullptr));
    const uint32_t nev = (uint32_t)x.n;
    if (nS < x.ns_min || nS > x.ns_max) return fail(c, SVT_EDEVICE, "%s: the counts disagree", t.what);
    if ((s = nomem(c, ix.d_ev.reserve(std::max<uint32_t>(nev, 1u)), t.mem))) return s;
    f.ev = ix.d_ev;
    f.n_ev = nev;
    file(f);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(e1, nullptr));
    HIP_TRY(c, hipEventSynchronize(e1));
    uint32_t err = 0;
    HIP_TRY(c, hipMemcpy(&err, f.err, 4, hipMemcpyDeviceToHost));
    if (err) return fail(c, SVT_EDEVICE, "%s: the filing disagrees with its count", t.what);
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, e0, e1));
    *build_ms = ms;
    ix.events[0] = nS;
    ix.events[1] = nev - nS;
    ix.built = true;
    return SVT_OK;
}

}  // namespace
}  // extern "C++"
