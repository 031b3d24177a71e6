// svt_loadprep.h -- the host pass of a pileup load (svt_load_host.inc), free of HIP: plain C++17, std
// only, so that it compiles on its own for the CPU model test (tests/test_loadprep_model.py) and under
// the sanitizers (tests/san/loadprep_san.cpp).  It validates the caller's arrays -- they are untrusted
// -- and builds what the uploads send: the prefix-max endpos, the records, the read buckets, the index
// ranges and the 64-read groups.  It defines no constants: the engine passes its own in Limits.
//
// Both functions return the rejection's message, or null.  prep() never reads the CIGAR stream;
// stream_prep() reads it for the clip bits when the caller gives none, and copies it when a read
// without ops needs its 0M word.
#ifndef SVT_LOADPREP_H
#define SVT_LOADPREP_H

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

namespace loadprep {

// Run fn(k) for k = 0 .. n-1 on up to `cap` threads (the host pass is per contig).
template <typename F>
void parallel_for(size_t n, size_t cap, F fn) {
    const size_t T = std::max<size_t>(1, std::min<size_t>({n, cap, (size_t)std::max(1u, std::thread::hardware_concurrency())}));
    if (T <= 1) {
        for (size_t k = 0; k < n; k++) fn(k);
        return;
    }
    std::atomic<size_t> next{0};
    std::vector<std::thread> th;
    for (size_t t = 0; t < T; t++)
        th.emplace_back([&] {
            for (size_t k; (k = next.fetch_add(1)) < n;) fn(k);
        });
    for (auto &x : th) x.join();
}

struct Limits {
    int bkt_shift;          // read-start bucket = 1 << bkt_shift bp
    uint32_t ncig_mask;     // a read's ops (nc's low bits; its clip bits are nc >> 30)
    uint32_t op_soft;       // the CIGAR op code of a soft clip
    int64_t wave;           // reads per group of the lane-per-read index
    int64_t rcap;           // reads per index range at most
    uint64_t t_min, t_max;  // bounds on the ops per index range
    uint64_t ix_ranges;     // index ranges aimed at per pileup
    uint64_t group_ops;     // a group with this many ops or more: no lane-per-read index (n_groups = 0)
    size_t threads;         // thread cap of the per-contig passes
};

// The per-read columns: nc[r] = n_cigar | clip << 30, soff[0..nr] the reads' offsets in the CIGAR
// stream (a read without ops owns one 0M word).
struct Reads {
    int32_t nt;
    const int64_t *tid_off;   // [nt + 1]
    const int32_t *pos, *endpos;
    const uint32_t *nc;
    const uint64_t *soff;
};

struct Rec {   // the device's uint4 record
    uint32_t pos, endpos, nc, tid;
};
struct Bkt {   // the device's uint2: {first contig-relative read with pos >= b << bkt_shift, first with emax >= it}
    uint32_t by_pos, by_emax;
};

struct Prep {
    std::vector<int32_t> emax;      // [nr] prefix max of endpos within the contig
    std::vector<Rec> rec;           // [nr]
    std::vector<uint8_t> clip8;     // [max(nr, 1)] nc >> 30
    std::vector<Bkt> bkt;           // every contig's read buckets, contig t's from bkt_off[t]
    std::vector<int64_t> bkt_off;   // [nt + 1]
    std::vector<uint64_t> part;     // [n_ranges + 1] first read of every index range, then nr
    std::vector<int64_t> vtop;      // [nt] per contig its largest pos / endpos (the value buckets)
    uint32_t n_ranges = 0;
    uint32_t n_groups = 0;          // 64-read groups of the lane-per-read index (0: a group too large for it)
};

inline const char *prep(const Limits &L, const Reads &in, Prep &out) {
    const int32_t nt = in.nt;
    const int64_t *tid_off = in.tid_off;
    const int32_t *pos = in.pos, *endpos = in.endpos;
    const uint32_t *nc = in.nc;
    const uint64_t *soff = in.soff;
    const int64_t nr = nt ? tid_off[nt] : 0;
    const uint64_t nstream = nr > 0 ? soff[nr] : 0;
    // ---- per contig in parallel: validation, prefix-max endpos, records, buckets
    out.emax.assign((size_t)nr, 0);
    out.rec.assign((size_t)nr, Rec{});
    out.clip8.assign((size_t)std::max<int64_t>(nr, 1), 0);
    out.vtop.assign((size_t)nt, 0);
    std::vector<int32_t> &emax = out.emax;
    std::vector<std::vector<Bkt>> bk((size_t)nt);
    std::vector<const char *> bad((size_t)nt, nullptr);
    parallel_for((size_t)nt, L.threads, [&](size_t t) {
        const int64_t r0 = tid_off[t], r1 = tid_off[t + 1];
        if (r1 - r0 > 0xffffffffll) { bad[t] = "> 2^32 reads on one contig"; return; }
        int32_t m = INT32_MIN, maxpos = 0;
        for (int64_t r = r0; r < r1; r++) {
            if (r > r0 && pos[r] < pos[r - 1]) { bad[t] = "reads not sorted by pos within a contig"; return; }
            if (pos[r] < 0 || endpos[r] <= pos[r]) { bad[t] = "pos < 0 or endpos <= pos"; return; }
            const uint64_t w = soff[r + 1] - soff[r], n = nc[r] & L.ncig_mask;
            if (soff[r + 1] < soff[r] || soff[r + 1] > nstream || w != std::max<uint64_t>(n, 1)) {
                bad[t] = "bad cig_off";
                return;
            }
            if (endpos[r] > m) m = endpos[r];
            maxpos = std::max(maxpos, pos[r]);
            emax[(size_t)r] = m;
            out.rec[(size_t)r] = Rec{(uint32_t)pos[r], (uint32_t)endpos[r], nc[r], (uint32_t)t};
            out.clip8[(size_t)r] = (uint8_t)(nc[r] >> 30);
        }
        // bucket b = 0..nb-1; the last bucket lies past every pos and endpos: {nr, nr}
        const int64_t top = r1 > r0 ? std::max<int64_t>(maxpos, m) : 0;
        out.vtop[t] = top;
        const int64_t nb = (top >> L.bkt_shift) + 2;
        std::vector<Bkt> &B = bk[t];
        B.reserve((size_t)nb);
        int64_t rp = r0, re = r0;
        for (int64_t b = 0; b < nb; b++) {
            const int64_t x = b << L.bkt_shift;
            while (rp < r1 && (int64_t)pos[rp] < x) rp++;
            while (re < r1 && (int64_t)emax[(size_t)re] < x) re++;
            B.push_back(Bkt{(uint32_t)(rp - r0), (uint32_t)(re - r0)});
        }
    });
    for (int32_t t = 0; t < nt; t++)
        if (bad[(size_t)t]) return bad[(size_t)t];
    out.bkt_off.assign((size_t)nt + 1, 0);
    for (int32_t t = 0; t < nt; t++) out.bkt_off[(size_t)t + 1] = out.bkt_off[(size_t)t] + (int64_t)bk[(size_t)t].size();
    out.bkt.assign((size_t)out.bkt_off[(size_t)nt], Bkt{});
    parallel_for((size_t)nt, L.threads, [&](size_t t) { std::copy(bk[t].begin(), bk[t].end(), out.bkt.begin() + out.bkt_off[t]); });
    // ---- ranges of the index build: ~T stream ops each, cut at read starts and contig starts, of at
    // most rcap reads (the single-pass walk stages their offsets)
    const uint64_t T = std::min<uint64_t>(std::max<uint64_t>(nstream / L.ix_ranges, L.t_min), L.t_max);
    std::vector<std::vector<uint64_t>> pt((size_t)nt);
    parallel_for((size_t)nt, L.threads, [&](size_t t) {
        for (int64_t r = tid_off[t], r1 = tid_off[t + 1]; r < r1;) {
            pt[t].push_back((uint64_t)r);
            const uint64_t s0 = soff[r];
            const int64_t rs = r;
            for (r++; r < r1 && soff[r] - s0 < T && r - rs < L.rcap; r++) {}
        }
    });
    out.part.clear();
    for (int32_t t = 0; t < nt; t++) out.part.insert(out.part.end(), pt[(size_t)t].begin(), pt[(size_t)t].end());
    out.part.push_back((uint64_t)nr);
    if (out.part.size() - 1 > 0x7fffffffull) return "too many index ranges";
    out.n_ranges = (uint32_t)(out.part.size() - 1);
    // the lane-per-read index's groups: each group's ops below group_ops, so that its events fit the
    // 32-bit wave scans and buffer sizes (else the stream walk builds the index)
    out.n_groups = (uint32_t)((nr + L.wave - 1) / L.wave);
    for (int64_t g0 = 0; g0 < nr && out.n_groups; g0 += L.wave)
        if (soff[std::min<int64_t>(g0 + L.wave, nr)] - soff[g0] >= L.group_ops) out.n_groups = 0;
    return nullptr;
}

// A caller's pileup as svt_load_pileup takes it.
struct View {
    int32_t nt;
    const int64_t *tid_off;
    const int32_t *pos, *endpos;
    const uint64_t *cig_off;
    const uint32_t *cigar;
    const uint8_t *clip;   // or null: the clip bits from each read's first and last CIGAR word
};

struct Stream {
    std::vector<uint32_t> nc;       // [nr] n_cigar | clip << 30
    uint64_t nops = 0;              // the caller's ops
    const uint64_t *soff = nullptr; // the stream prep() and the index walk: the caller's arrays, or the
    const uint32_t *words = nullptr;//   two below when some read has no ops
    std::vector<uint64_t> soff2;
    std::vector<uint32_t> words2;
};

inline const char *stream_prep(const Limits &L, const View &p, Stream &out) {
    const int32_t nt = p.nt;
    const int64_t nr = nt ? p.tid_off[nt] : 0;
    if (nt && p.tid_off[0] != 0) return "tid_off[0] != 0";
    for (int32_t t = 0; t < nt; t++)
        if (p.tid_off[t + 1] < p.tid_off[t]) return "tid_off not monotone";
    if (nr > 0 && (!p.pos || !p.endpos || !p.cig_off || (!p.cigar && p.cig_off[nr] > 0))) return "missing arrays";
    const uint64_t nops = nr > 0 ? p.cig_off[nr] : 0;
    if (nr > 0 && p.cig_off[0] != 0) return "cig_off[0] != 0";
    out.nops = nops;
    // per read n_cigar | clip << 30 (clip from the caller, or from the CIGAR words)
    out.nc.assign((size_t)nr, 0);
    std::vector<int64_t> zeros((size_t)std::max(nt, 1), 0);   // reads with n_cigar == 0 per contig
    std::vector<const char *> bad((size_t)std::max(nt, 1), nullptr);
    parallel_for((size_t)nt, L.threads, [&](size_t t) {
        for (int64_t r = p.tid_off[t], r1 = p.tid_off[t + 1]; r < r1; r++) {
            const uint64_t o0 = p.cig_off[r], o1 = p.cig_off[r + 1];
            if (o1 < o0 || o1 > nops || o1 - o0 > L.ncig_mask) { bad[t] = "bad cig_off"; return; }
            const uint32_t ncig = (uint32_t)(o1 - o0);
            uint32_t clip;
            if (p.clip) clip = p.clip[r] & 3u;
            else clip = ncig ? (((p.cigar[o1 - 1] & 0xfu) == L.op_soft ? 1u : 0u) |
                                ((p.cigar[o0] & 0xfu) == L.op_soft ? 2u : 0u)) : 0u;
            zeros[t] += ncig == 0;
            out.nc[(size_t)r] = ncig | clip << 30;
        }
    });
    for (int32_t t = 0; t < nt; t++)
        if (bad[(size_t)t]) return bad[(size_t)t];
    // ---- the CIGAR stream: the caller's words; a read with n_cigar == 0 gets one 0M word (no
    // advance, never a candidate) so that every read owns a stream op (svt_index.inc)
    int64_t nzero = 0;
    for (int32_t t = 0; t < nt; t++) nzero += zeros[(size_t)t];
    out.soff = p.cig_off;
    out.words = p.cigar;
    out.soff2.clear();
    out.words2.clear();
    if (nzero > 0) {
        out.soff2.resize((size_t)nr + 1);
        out.words2.reserve(nops + (uint64_t)nzero);
        for (int64_t r = 0; r < nr; r++) {
            out.soff2[(size_t)r] = out.words2.size();
            const uint64_t o0 = p.cig_off[r], o1 = p.cig_off[r + 1];
            if (o1 == o0) out.words2.push_back(0u);
            else out.words2.insert(out.words2.end(), p.cigar + o0, p.cigar + o1);
        }
        out.soff2[(size_t)nr] = out.words2.size();
        out.soff = out.soff2.data();
        out.words = out.words2.data();
    }
    return nullptr;
}

}  // namespace loadprep

#endif
