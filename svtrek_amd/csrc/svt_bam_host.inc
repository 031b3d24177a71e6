// svt_bam_host.inc -- host half of the device BAM decoder (included last by svt_engine.hip):
// svt_bam_dec and the svt_bam_dec_* entry points.  The kernels are in svt_bam.inc and
// svt_inflate.inc.


// svt_bam_dec_feed is pipelined one batch deep: a call copies its batch's compressed bytes to the
// device (a copy stream, into one of two input buffers) while the previous batch still inflates,
// then decodes the previous batch (whose carried tail fixes where this batch's bytes go) and
// launches this batch's inflate; the next call or svt_bam_dec_load decodes it.  (Copying a batch in
// parts beside its own inflate measured slower: every part's launch waits for its slowest block,
// profiles/r05_I.)
struct svt_bam_dec {
    svt_ctx *c = nullptr;
    int32_t n_ref = 0;
    hipStream_t st = nullptr;
    hipStream_t cst = nullptr;                // the copy stream
    DevEvent cev;                             // the latest batch's bytes are on the device
    DevBuf<uint8_t> d_comp[2];                // compressed batches (alternating)
    DevBuf<svt_bgzf_block> d_blk[2];
    int ib = 0;                               // the next batch's input buffer
    DevBuf<uint32_t> d_err;                   // the inflate's first bad block (this decoder's own word)
    bool pend = false;                        // a batch inflated (or inflating) but not yet decoded
    size_t pend_n = 0;
    uint64_t pend_u = 0, pend_r0 = 0;
    DevBuf<uint8_t> d_buf[2];                 // inflated batches: [carried tail | this batch]
    int cur = 0;
    uint64_t tail = 0;                        // bytes of the incomplete record at the front of d_buf[cur]
    bool first = true;
    DevBuf<BdChunk> d_ch;
    DevBuf<uint32_t> d_base;
    DevBuf<BdRec> d_rec;
    DevBuf<BdTot> d_pre;
    DevBuf<BdCheck> d_chk;
    DevBuf<uint8_t> d_tmp;                    // hipcub's temporary storage
    // the columns (one entry per kept read, each grown by its own capacity) and the CIGAR stream:
    // what BdCols points at (bd_cols)
    DevBuf<int32_t> d_tid, d_pos, d_endpos;
    DevBuf<uint32_t> d_nc;
    DevBuf<uint64_t> d_soff;
    DevBuf<uint32_t> d_stream;                // handed to the context by svt_bam_dec_load
    uint64_t nkept = 0, nwords = 0;
    svt_bam_dec_stats stats{};
};
static_assert(!std::is_copy_constructible<svt_bam_dec>::value, "a decoder owns its device memory");

namespace {
// A failed growth of one of the decoder's buffers (allocation or the copy of what it held).
svt_status bd_mem(svt_ctx *c, hipError_t e) { return nomem(c, e, "device memory for the BAM decode"); }

BdCols bd_cols(const svt_bam_dec *d) { return BdCols{d->d_tid, d->d_pos, d->d_endpos, d->d_nc, d->d_soff, d->d_stream}; }
}  // namespace

extern "C" {

svt_status svt_bam_dec_open(svt_ctx *c, int32_t n_targets, svt_bam_dec **out) {
    if (!c || !out || n_targets < 0) return SVT_EINVAL;
    *out = nullptr;
    DEV_GUARD(c);
    svt_bam_dec *d = new (std::nothrow) svt_bam_dec();
    if (!d) return fail(c, SVT_ENOMEM, "%s", "host memory");
    d->c = c;
    d->n_ref = n_targets;
    const bool ok = hipStreamCreateWithFlags(&d->st, hipStreamNonBlocking) == hipSuccess &&
                    hipStreamCreateWithFlags(&d->cst, hipStreamNonBlocking) == hipSuccess &&
                    d->cev.create(hipEventDisableTiming) == hipSuccess && d->d_chk.reserve(1) == hipSuccess &&
                    d->d_err.reserve(1) == hipSuccess;
    if (!ok) {
        svt_bam_dec_close(d);
        return fail(c, SVT_EDEVICE, "%s", "BAM decode: stream / buffers");
    }
    *out = d;
    return SVT_OK;
}

namespace {
// The pending batch's records: it was inflated into d_buf[cur] after the carried tail (its
// kernels run on d->st, so the decode's launches wait for them).  The incomplete last record
// moves to the front of the other buffer.
svt_status bd_decode(svt_bam_dec *d) {
    svt_ctx *c = d->c;
    svt_status s;
    d->pend = false;
    uint8_t *buf = d->d_buf[d->cur];
    const uint64_t N = d->tail + d->pend_u, r0 = d->pend_r0;
    const uint64_t span = N - r0;
    const uint32_t nch = (uint32_t)((span + BD_CHUNK - 1) / BD_CHUNK);
    BdCheck chk{1u, 0u, 0ull, N, 0u, 0u, 0ull};
    if (nch) {
        if ((s = bd_mem(c, d->d_ch.grow(nch))) || (s = bd_mem(c, d->d_base.grow(nch)))) return s;
        hipLaunchKernelGGL(bd_chunk_kernel, dim3(nch), dim3(WAVE), 0, d->st, buf, r0, N, nch, d->n_ref, d->d_ch);
        hipLaunchKernelGGL(bd_check_kernel, dim3(1), dim3(WAVE), 0, d->st, buf, d->d_ch, nch, r0, N, d->d_chk);
        HIP_TRY(c, hipGetLastError());
        uint32_t ierr = 0xffffffffu;
        HIP_TRY(c, hipMemcpyAsync(&chk, d->d_chk, sizeof chk, hipMemcpyDeviceToHost, d->st));
        HIP_TRY(c, hipMemcpyAsync(&ierr, d->d_err, sizeof ierr, hipMemcpyDeviceToHost, d->st));
        HIP_TRY(c, hipStreamSynchronize(d->st));
        if (d->pend_n && ierr != 0xffffffffu) {
            char m[64];
            snprintf(m, sizeof m, "%u", ierr);
            return fail(c, SVT_EINVAL, "corrupt BGZF block %s of the batch (does not inflate to its ISIZE)", m);
        }
        if (!chk.ok) {   // a wrong guess: the exact chain, hop by hop from the first wrong chunk on
            d->stats.rechained++;
            d->stats.rechained_chunks += nch - chk.kfail;
            hipLaunchKernelGGL(bd_chain_kernel, dim3(1), dim3(WAVE), 0, d->st, buf, r0, N, nch, chk.kfail, chk.efail,
                               d->d_ch);
            hipLaunchKernelGGL(bd_check_kernel, dim3(1), dim3(WAVE), 0, d->st, buf, d->d_ch, nch, r0, N, d->d_chk);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipMemcpyAsync(&chk, d->d_chk, sizeof chk, hipMemcpyDeviceToHost, d->st));
            HIP_TRY(c, hipStreamSynchronize(d->st));
            if (!chk.ok) return fail(c, SVT_EDEVICE, "%s", "BAM decode: the exact record chain failed its own check");
        }
        if (chk.bad) return fail(c, SVT_EINVAL, "%s", "corrupt BAM record (block_size < 32)");
    }
    if (chk.nrec) {
        const uint64_t nrec = chk.nrec;
        if (nrec >= 0xffffffffull) return fail(c, SVT_EINVAL, "%s", "BAM decode: more than 2^32 records in one batch");
        if ((s = bd_mem(c, d->d_rec.grow(nrec))) || (s = bd_mem(c, d->d_pre.grow(nrec)))) return s;
        // the chunks' record counts -> their first record's index; the records; their kept / word prefixes
        const auto cnt = hipcub::TransformInputIterator<uint32_t, BdCntOf, const BdChunk *>(d->d_ch, BdCntOf());
        const auto tot = hipcub::TransformInputIterator<BdTot, BdTotOf, const BdRec *>(d->d_rec, BdTotOf());
        size_t need1 = 0, need2 = 0;
        HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, need1, cnt, d->d_base.get(), (int)chk.nk, d->st));
        HIP_TRY(c, hipcub::DeviceScan::ExclusiveScan(nullptr, need2, tot, d->d_pre.get(), BdTotSum(), BdTot{0, 0, 0, 0, 0},
                                                     (int)nrec, d->st));
        if ((s = bd_mem(c, d->d_tmp.grow(std::max(need1, need2))))) return s;
        size_t t1 = d->d_tmp.cap(), t2 = d->d_tmp.cap();
        HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(d->d_tmp.get(), t1, cnt, d->d_base.get(), (int)chk.nk, d->st));
        hipLaunchKernelGGL(bd_rec_kernel, dim3(chk.nk), dim3(WAVE), 0, d->st, buf, d->d_ch, d->d_base, chk.nk, d->n_ref,
                           d->d_rec);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipcub::DeviceScan::ExclusiveScan(d->d_tmp.get(), t2, tot, d->d_pre.get(), BdTotSum(), BdTot{0, 0, 0, 0, 0},
                                                     (int)nrec, d->st));
        BdTot last{};
        BdRec lr{};
        HIP_TRY(c, hipMemcpyAsync(&last, d->d_pre + nrec - 1, sizeof last, hipMemcpyDeviceToHost, d->st));
        HIP_TRY(c, hipMemcpyAsync(&lr, d->d_rec + nrec - 1, sizeof lr, hipMemcpyDeviceToHost, d->st));
        HIP_TRY(c, hipStreamSynchronize(d->st));
        const BdTot all = BdTotSum()(last, BdTotOf()(lr));
        if (all.bad) return fail(c, SVT_EINVAL, "%s", "corrupt BAM record");
        // the columns and the stream (STREAM_PAD spare words), grown keeping what they hold
        const uint64_t G = d->nkept + all.keep + 1, W = d->nwords + all.words + STREAM_PAD;
        if ((s = bd_mem(c, d->d_tid.grow(G, d->nkept))) || (s = bd_mem(c, d->d_pos.grow(G, d->nkept))) ||
            (s = bd_mem(c, d->d_endpos.grow(G, d->nkept))) || (s = bd_mem(c, d->d_nc.grow(G, d->nkept))) ||
            (s = bd_mem(c, d->d_soff.grow(G, d->nkept))) || (s = bd_mem(c, d->d_stream.grow(W, d->nwords))))
            return s;
        hipLaunchKernelGGL(bd_copy_kernel, dim3((unsigned)std::min<uint64_t>((nrec + 3) / 4, 16384)), dim3(256), 0, d->st,
                           buf, d->d_rec, d->d_pre, nrec, bd_cols(d), d->nkept, d->nwords);
        HIP_TRY(c, hipGetLastError());
        d->nkept += all.keep;
        d->nwords += all.words;
        d->stats.records += nrec;
        d->stats.reads += all.keep;
        d->stats.cigar_ops += all.ops;
        d->stats.cg_restored += all.cg;
    }
    // the incomplete last record moves to the front of the other buffer
    const uint64_t nt = N - chk.tail;
    int nx = d->cur ^ 1;
    if ((s = bd_mem(c, d->d_buf[nx].grow(std::max<uint64_t>(nt, 1) + 64)))) return s;
    if (nt) HIP_TRY(c, hipMemcpyAsync(d->d_buf[nx], buf + chk.tail, nt, hipMemcpyDeviceToDevice, d->st));
    HIP_TRY(c, hipStreamSynchronize(d->st));
    d->cur = nx;
    d->tail = nt;
    return SVT_OK;
}
}  // namespace

svt_status svt_bam_dec_feed(svt_bam_dec *d, const uint8_t *comp, size_t comp_bytes, const svt_bgzf_block *blocks,
                            size_t n, uint64_t skip) {
    if (!d) return SVT_EINVAL;
    svt_ctx *c = d->c;
    if (n && (!comp || !blocks)) return fail(c, SVT_EINVAL, "%s", "null buffer");
    if (n > 0xfffffffeull) return fail(c, SVT_EINVAL, "%s", "more than 2^32 - 2 blocks in one call");
    uint64_t U = 0, lo = ~0ull, hi = 0;
    for (size_t i = 0; i < n; i++) {   // every block inside its buffers (the kernel trusts the table)
        const svt_bgzf_block &k = blocks[i];
        if (k.clen > 65536u || k.ulen > 65536u || k.coff > comp_bytes || k.clen > comp_bytes - k.coff)
            return fail(c, SVT_EINVAL, "%s", "BGZF block outside its buffers (or over 64 KiB)");
        U = std::max<uint64_t>(U, k.uoff + k.ulen);
        lo = std::min<uint64_t>(lo, k.coff);
        hi = std::max<uint64_t>(hi, k.coff + k.clen);
    }
    DEV_GUARD(c);
    using clk = std::chrono::steady_clock;
    const clk::time_point t0 = clk::now();
    svt_status s;
    const uint64_t r0 = d->first ? skip : 0;   // (the first batch carries no tail)
    if (r0 > (d->first ? 0 : d->tail) + U) return fail(c, SVT_EINVAL, "%s", "BAM decode: the header runs past the first batch");
    d->first = false;
    // this batch's bytes cross PCIe while the previous batch inflates (its input is the other buffer)
    const int ib = d->ib;
    d->ib ^= 1;
    if ((s = bd_mem(c, d->d_comp[ib].grow(comp_bytes + 64))) || (s = bd_mem(c, d->d_blk[ib].grow(std::max<size_t>(n, 1)))))
        return s;
    // Once this batch's copies are queued, every return waits for them first: the header lets the
    // caller reuse `comp` / `blocks` as soon as the call returns, error returns included.
    struct CopyWait {
        hipStream_t cst = nullptr;
        ~CopyWait() {
            if (cst) (void)hipStreamSynchronize(cst);
        }
    } copy_wait;
    if (n) {
        copy_wait.cst = d->cst;
        HIP_TRY(c, hipMemcpyAsync(d->d_blk[ib], blocks, n * sizeof(svt_bgzf_block), hipMemcpyHostToDevice, d->cst));
        if (hi > lo) HIP_TRY(c, hipMemcpyAsync(d->d_comp[ib] + lo, comp + lo, hi - lo, hipMemcpyHostToDevice, d->cst));
        HIP_TRY(c, hipEventRecord(d->cev, d->cst));
    }
    // the previous batch's records: fixes the carried tail this batch's bytes follow
    if (d->pend && (s = bd_decode(d))) return s;
    const uint64_t T = d->tail, N = T + U;
    if ((s = bd_mem(c, d->d_buf[d->cur].grow(N + 64, T)))) return s;
    if (n) {
        if ((s = order_on(c, d->st))) return s;
        HIP_TRY(c, hipMemsetAsync(d->d_err, 0xff, sizeof(uint32_t), d->st));
        HIP_TRY(c, hipStreamWaitEvent(d->st, d->cev, 0));
        const unsigned grid = (unsigned)std::min<size_t>(n, (size_t)INF_GRID);
        hipLaunchKernelGGL(inflate_kernel, dim3(grid), dim3(WAVE), 0, d->st, d->d_comp[ib], d->d_blk[ib], 0u, (uint32_t)n,
                           d->d_buf[d->cur] + T, d->d_err);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventSynchronize(d->cev));   // the caller may reuse its buffers
        copy_wait.cst = nullptr;
    }
    d->pend = true;
    d->pend_n = n;
    d->pend_u = U;
    d->pend_r0 = r0;
    d->stats.batches++;
    d->stats.inflated_bytes += U;
    d->stats.feed_ms += std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    return SVT_OK;
}

svt_status svt_bam_dec_stats_get(const svt_bam_dec *d, svt_bam_dec_stats *out) {
    if (!d || !out) return SVT_EINVAL;
    *out = d->stats;
    return SVT_OK;
}

namespace {
// svt_bam_dec_load's body inside load_frame (t0: the frame's start): the decoded columns to the host,
// then the host pass and the rest of the load by load_core.
svt_status bd_load(svt_bam_dec *d, LoadClock::time_point t0) {
    svt_ctx *c = d->c;
    const int32_t nt = d->n_ref;
    const uint64_t n = d->nkept;
    svt_status s;
    // sortedness and the contig boundaries, on the device
    DevBuf<int64_t> d_toff;
    DevBuf<uint32_t> d_uns;
    HIP_TRY(c, d_toff.reserve((size_t)nt + 1));
    if ((s = nomem(c, d_uns.reserve(1), "device"))) return s;
    std::vector<int64_t> toff((size_t)nt + 1, 0);
    uint32_t uns = 0;
    HIP_TRY(c, hipMemsetAsync(d_uns, 0, sizeof(uint32_t), d->st));
    HIP_TRY(c, hipMemsetAsync(d_toff, 0, ((size_t)nt + 1) * sizeof(int64_t), d->st));
    const unsigned g = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 256) / 256, 65536));
    hipLaunchKernelGGL(bd_finish_kernel, dim3(g), dim3(256), 0, d->st, d->d_tid, d->d_pos, n, nt, d_toff, d_uns);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(toff.data(), d_toff, toff.size() * sizeof(int64_t), hipMemcpyDeviceToHost, d->st));
    HIP_TRY(c, hipMemcpyAsync(&uns, d_uns, sizeof uns, hipMemcpyDeviceToHost, d->st));
    HIP_TRY(c, hipStreamSynchronize(d->st));
    d_toff.reset();
    d_uns.reset();
    // the per-read columns the host pass reads (pos, endpos, n_cigar | clip, stream offsets)
    std::vector<int32_t> pos(n), endpos(n), tid(uns ? n : 0);
    std::vector<uint32_t> nc(n);
    std::vector<uint64_t> soff(n + 1);
    if (n) {
        HIP_TRY(c, hipMemcpy(pos.data(), d->d_pos, n * 4, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(endpos.data(), d->d_endpos, n * 4, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(nc.data(), d->d_nc, n * 4, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(soff.data(), d->d_soff, n * 8, hipMemcpyDeviceToHost));
        if (uns) HIP_TRY(c, hipMemcpy(tid.data(), d->d_tid, n * 4, hipMemcpyDeviceToHost));
    }
    soff[n] = d->nwords;
    const double pre = ms_since(t0);
    if (uns) {   // not coordinate-sorted: sort on the host (stable, by tid then pos), as the host ingest does
        std::vector<uint32_t> strm(d->nwords);
        if (d->nwords) HIP_TRY(c, hipMemcpy(strm.data(), d->d_stream, d->nwords * 4, hipMemcpyDeviceToHost));
        std::vector<size_t> idx(n);
        for (size_t i = 0; i < n; i++) idx[i] = i;
        std::stable_sort(idx.begin(), idx.end(), [&](size_t x, size_t y) {
            return tid[x] != tid[y] ? tid[x] < tid[y] : pos[x] < pos[y];
        });
        std::vector<int32_t> p2(n), e2(n);
        std::vector<uint32_t> n2(n), s2;
        std::vector<uint64_t> o2(n + 1);
        s2.reserve(d->nwords);
        std::fill(toff.begin(), toff.end(), 0);
        for (size_t k = 0; k < n; k++) {
            const size_t i = idx[k];
            p2[k] = pos[i]; e2[k] = endpos[i]; n2[k] = nc[i];
            o2[k] = s2.size();
            s2.insert(s2.end(), strm.begin() + (ptrdiff_t)soff[i], strm.begin() + (ptrdiff_t)soff[i + 1]);
            toff[(size_t)tid[i] + 1]++;
        }
        o2[n] = s2.size();
        for (int32_t t = 0; t < nt; t++) toff[(size_t)t + 1] += toff[(size_t)t];
        return load_core(c, loadprep::Reads{nt, toff.data(), p2.data(), e2.data(), n2.data(), o2.data()}, s2.data(), nullptr,
                         d->stats.cigar_ops, pre);
    }
    // the stream stays where the decode wrote it (its spare words zeroed): the context adopts it;
    // a BAM without records never allocated one, so it gets just the spare words here
    if ((s = bd_mem(c, d->d_stream.grow(d->nwords + STREAM_PAD, d->nwords)))) return s;
    HIP_TRY(c, hipMemset(d->d_stream + d->nwords, 0, STREAM_PAD * 4));
    return load_core(c, loadprep::Reads{nt, toff.data(), pos.data(), endpos.data(), nc.data(), soff.data()}, nullptr,
                     &d->d_stream, d->stats.cigar_ops, pre);
}
}  // namespace

svt_status svt_bam_dec_load(svt_bam_dec *d) {
    if (!d) return SVT_EINVAL;
    svt_ctx *c = d->c;
    DEV_GUARD(c);
    using clk = std::chrono::steady_clock;
    if (d->pend) {   // the last batch's records
        const clk::time_point tf = clk::now();
        const svt_status sd = bd_decode(d);
        d->stats.feed_ms += std::chrono::duration<double, std::milli>(clk::now() - tf).count();
        if (sd) return sd;
    }
    if (d->tail) return fail(c, SVT_EINVAL, "%s", "truncated BAM record at end of file");
    return load_frame(c, [&](LoadClock::time_point t0) { return bd_load(d, t0); });
}

void svt_bam_dec_close(svt_bam_dec *d) {
    if (!d) return;
    {
        DevGuard dg(d->c->device);
        if (d->st) (void)hipStreamSynchronize(d->st);
        // the context's launch order may point at this stream (svt_bam_dec_feed's order_on): all of
        // its work is done, so nothing later has to wait for it, and it must not be named again
        if (d->c->have_last && d->c->last_stream == d->st) d->c->have_last = false;
        if (d->cst) (void)hipStreamSynchronize(d->cst);
        if (d->st) (void)hipStreamDestroy(d->st);
        if (d->cst) (void)hipStreamDestroy(d->cst);
        delete d;   // its buffers and its event go with it, on the context's device
    }
}

}  // extern "C"
