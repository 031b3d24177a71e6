// loadprep_shim.cpp -- svt_loadprep.h behind a C interface for tests/test_loadprep_model.py (ctypes), and the
// seeded run whose digest tests/san/loadprep_san.cpp prints under the sanitizers.
#include <stdio.h>
#include <string.h>

#include <string>

#include "svt_loadprep.h"

namespace {

// lim[10]: bkt_shift, ncig_mask, op_soft, wave, rcap, t_min, t_max, ix_ranges, group_ops, threads
loadprep::Limits limits(const int64_t *lim) {
    return loadprep::Limits{(int)lim[0], (uint32_t)lim[1], (uint32_t)lim[2], lim[3], lim[4], (uint64_t)lim[5],
                            (uint64_t)lim[6], (uint64_t)lim[7], (uint64_t)lim[8], (size_t)lim[9]};
}

struct Run {
    loadprep::Prep p;
    loadprep::Stream s;
    const char *err = nullptr;
};

struct Span {
    const void *p;
    size_t bytes;
};

template <typename T>
Span span(const std::vector<T> &v) { return Span{v.data(), v.size() * sizeof(T)}; }

Span array(const Run &r, int which) {
    switch (which) {
    case 0: return span(r.p.emax);
    case 1: return span(r.p.rec);
    case 2: return span(r.p.clip8);
    case 3: return span(r.p.bkt);
    case 4: return span(r.p.bkt_off);
    case 5: return span(r.p.part);
    case 6: return span(r.p.vtop);
    case 7: return span(r.s.nc);
    case 8: return Span{r.s.soff, r.s.soff && !r.s.nc.empty() ? (r.s.nc.size() + 1) * sizeof(uint64_t) : 0};
    case 9: return Span{r.s.words, r.s.soff && !r.s.nc.empty() ? (size_t)r.s.soff[r.s.nc.size()] * sizeof(uint32_t) : 0};
    default: return Span{nullptr, 0};
    }
}
const char *const NAMES[10] = {"emax", "rec", "clip8", "bkt", "bkt_off", "part", "vtop", "nc", "soff", "words"};

uint64_t fnv(Span s) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < s.bytes; i++) h = (h ^ ((const uint8_t *)s.p)[i]) * 1099511628211ull;
    return h;
}

}  // namespace

extern "C" {

void *lp_prep(const int64_t *lim, int32_t nt, const int64_t *tid_off, const int32_t *pos, const int32_t *endpos,
              const uint32_t *nc, const uint64_t *soff) {
    Run *r = new Run();
    r->err = loadprep::prep(limits(lim), loadprep::Reads{nt, tid_off, pos, endpos, nc, soff}, r->p);
    return r;
}

void *lp_stream_prep(const int64_t *lim, int32_t nt, const int64_t *tid_off, const int32_t *pos, const int32_t *endpos,
                     const uint64_t *cig_off, const uint32_t *cigar, const uint8_t *clip) {
    Run *r = new Run();
    r->err = loadprep::stream_prep(limits(lim), loadprep::View{nt, tid_off, pos, endpos, cig_off, cigar, clip}, r->s);
    return r;
}

const char *lp_error(const void *h) { return ((const Run *)h)->err; }
uint64_t lp_bytes(const void *h, int which) { return array(*(const Run *)h, which).bytes; }
void lp_copy(const void *h, int which, void *dst) {
    const Span s = array(*(const Run *)h, which);
    if (s.bytes) memcpy(dst, s.p, s.bytes);
}
uint32_t lp_n_ranges(const void *h) { return ((const Run *)h)->p.n_ranges; }
uint32_t lp_n_groups(const void *h) { return ((const Run *)h)->p.n_groups; }
uint64_t lp_nops(const void *h) { return ((const Run *)h)->s.nops; }
void lp_free(void *h) { delete (Run *)h; }

// A seeded pileup of five contigs (one empty) and a few thousand reads, some without ops, through both
// functions -- the clip bits derived from the words, then given -- on `threads` threads.  Writes one
// "name digest bytes" line per output array into out[cap]; returns the text's length, or -1.
int lp_seeded_digest(uint64_t seed, int threads, char *out, int cap) {
    uint64_t x = seed * 0x9e3779b97f4a7c15ull + 1;
    auto rnd = [&](uint64_t n) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        return (x >> 11) % n;
    };
    const int32_t nt = 5;
    const int64_t per[nt] = {1500, 0, 700, 1, 1300};
    std::vector<int64_t> tid_off(nt + 1, 0);
    std::vector<int32_t> pos, endpos;
    std::vector<uint64_t> cig_off(1, 0);
    std::vector<uint32_t> cigar;
    std::vector<uint8_t> clip;
    for (int32_t t = 0; t < nt; t++) {
        int32_t p = 0;
        for (int64_t k = 0; k < per[t]; k++) {
            p += (int32_t)rnd(300);
            pos.push_back(p);
            endpos.push_back(p + 1 + (int32_t)rnd(rnd(20) ? 3000 : 40000));
            const uint64_t n = rnd(10) ? 1 + rnd(30) : 0;
            for (uint64_t i = 0; i < n; i++)
                cigar.push_back((uint32_t)(1 + rnd(400)) << 4 | (uint32_t)((i == 0 || i == n - 1) && rnd(3) == 0 ? 4 : rnd(3)));
            cig_off.push_back(cigar.size());
            clip.push_back((uint8_t)rnd(4));
        }
        tid_off[(size_t)t + 1] = tid_off[(size_t)t] + per[t];
    }
    if (cigar.empty()) cigar.push_back(0);
    // (256 ops a range at least, so that ranges end on the ops bound as well as on the 32-read bound)
    const int64_t lim[10] = {12, 0x1fffffff, 4, 64, 32, 256, 65536, 32768, 1 << 27, threads};
    std::string text;
    for (int given = 0; given < 2; given++) {
        Run r;
        r.err = loadprep::stream_prep(limits(lim), loadprep::View{nt, tid_off.data(), pos.data(), endpos.data(), cig_off.data(),
                                                                  cigar.data(), given ? clip.data() : nullptr}, r.s);
        if (!r.err)
            r.err = loadprep::prep(limits(lim), loadprep::Reads{nt, tid_off.data(), pos.data(), endpos.data(), r.s.nc.data(), r.s.soff}, r.p);
        if (r.err) return -1;
        char line[96];
        for (int w = 0; w < 10; w++) {
            const Span s = array(r, w);
            snprintf(line, sizeof line, "%d %s %016llx %zu\n", given, NAMES[w], (unsigned long long)fnv(s), s.bytes);
            text += line;
        }
        snprintf(line, sizeof line, "%d n_ranges %u n_groups %u nops %llu\n", given, r.p.n_ranges, r.p.n_groups,
                 (unsigned long long)r.s.nops);
        text += line;
    }
    if ((int)text.size() >= cap) return -1;
    memcpy(out, text.c_str(), text.size() + 1);
    return (int)text.size();
}

}  // extern "C"
