// jnclass_shim.cpp -- svt_jnclass.h behind a C interface for tests/test_jnclass_model.py (ctypes), and the two
// tables whose digest tests/san/jnclass_san.cpp prints under the sanitizers: a seeded fuzz table and the
// extreme-value table.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "svt_jnclass.h"

namespace {

constexpr int JC_FIELDS = 12;   // have, kind, other, past, tid, x, len, lo, hi, tid_hi, y, o

// lim[4]: min_len, x_sat, len_max, ext_max
JnLimits limits(const int64_t *lim) { return JnLimits{lim[0], (uint32_t)lim[1], (uint32_t)lim[2], (uint32_t)lim[3]}; }

struct Table {
    std::vector<uint64_t> off{0};
    std::vector<svt_junction_seg> seg;
    void row(int32_t tid, uint32_t strand, uint64_t r_beg, uint64_t r_end, uint64_t q_beg, uint64_t q_end) {
        seg.push_back(svt_junction_seg{tid, strand, (uint32_t)r_beg, (uint32_t)r_end, (uint32_t)q_beg, (uint32_t)q_end});
    }
    void end() { off.push_back(seg.size()); }
    uint64_t n() const { return off.size() - 1; }
};

struct Rng {
    uint64_t x;
    uint64_t operator()(uint64_t n) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        return (x >> 11) % n;
    }
    int64_t in(int64_t lo, int64_t hi) { return lo + (int64_t)(*this)((uint64_t)(hi - lo + 1)); }
};

// n records of 1-6 rows around an own segment A: the other rows' contig, strand and query start are drawn
// near A's, their reference coordinates so that the join's distance (dr, or p - q across strands) is one of
// the thresholds' neighbours or anything within 3 kb; a few records lie at 2^30 and below 2^32.
Table seeded(uint64_t seed, uint64_t n) {
    Rng rnd{seed * 0x9e3779b97f4a7c15ull + 1};
    Table t;
    static const int64_t EDGE[9] = {-51, -50, -49, -1, 0, 1, 49, 50, 51};
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t where = rnd(50);
        const int64_t base = where == 0 ? (1ll << 30) - 3000 + rnd.in(0, 6000) : where == 1 ? (1ll << 32) - 20000 + rnd.in(0, 2000)
                                                                                             : rnd.in(10000, 1000000);
        const int32_t tid = (int32_t)rnd(4);
        const uint32_t st = (uint32_t)rnd(2);
        const int64_t a_beg = base, a_end = base + rnd.in(100, 5000), aq_beg = rnd.in(0, 2000), aq_end = aq_beg + rnd.in(50, 3000);
        t.row(tid, st, a_beg, a_end, aq_beg, aq_end);
        const uint64_t extra = rnd(8) == 0 ? 0 : 1 + rnd(5);
        for (uint64_t e = 0; e < extra; e++) {
            if (rnd(50) == 0) {   // A's own tuple again
                t.row(tid, st, a_beg, a_end + rnd(3), aq_beg, aq_end);
                continue;
            }
            const int32_t btid = rnd(4) ? tid : (int32_t)rnd(4);
            const uint32_t bst = rnd(10) < 7 ? st : 1u - st;
            const uint64_t qm = rnd(10);
            const int64_t bq_beg = qm == 0 ? rnd.in(0, aq_beg) : qm == 1 ? aq_end - rnd.in(1, 30) : qm < 4 ? aq_end + rnd.in(0, 1)
                                   : qm < 6 ? aq_end + rnd.in(2, 3000) : aq_end + rnd.in(2, 300);
            const int64_t bq_end = bq_beg + rnd.in(50, 3000), rlen = rnd.in(100, 5000);
            const int64_t g = rnd(10) < 3 ? EDGE[rnd(9)] : rnd.in(-3000, 3000);
            int64_t b_beg;
            if (bst == st) b_beg = st ? a_beg - g - rlen : a_end + g;             // dr = g
            else {
                const int64_t q = (st ? a_beg : a_end) + g;                         // q - p = g
                b_beg = bst ? q - rlen : q;
            }
            t.row(btid, bst, b_beg, b_beg + rlen, bq_beg, bq_end);
        }
        t.end();
    }
    return t;
}

// Two-row records over every combination of the 32-bit fields' extremes in the four reference coordinates
// (r_end < r_beg included: the classifier must not depend on the loader's checks), both strands of both
// rows, the same contig and another one, B's query tuple later than A's in three ways.
Table extreme() {
    static const uint64_t V[7] = {0, 1, (1ull << 30) - 1, 1ull << 30, (1ull << 31) - 1, 1ull << 31, (1ull << 32) - 1};
    static const uint64_t Q[3][2] = {{11, (1ull << 32) - 1}, {(1ull << 32) - 1, (1ull << 32) - 1}, {0, 11}};
    Table t;
    uint64_t k = 0;
    for (uint64_t a0 : V)
        for (uint64_t a1 : V)
            for (uint64_t b0 : V)
                for (uint64_t b1 : V)
                    for (uint32_t s = 0; s < 4; s++)
                        for (int32_t tb = 0; tb < 3; tb++, k++) {   // A on contig 1: B on 0, 1, 2
                            t.row(1, s & 1u, a0, a1, 0, 10);
                            t.row(tb, s >> 1, b0, b1, Q[k % 3][0], Q[k % 3][1]);
                            t.end();
                        }
    return t;
}

void classify(const JnLimits &L, uint64_t n, const uint64_t *off, const svt_junction_seg *seg, int64_t *out) {
    for (uint64_t k = 0; k < n; k++) {
        int64_t *o = out + k * JC_FIELDS;
        svt_junction_seg A, B;
        memset(o, 0, JC_FIELDS * sizeof *o);
        if (!jn_next(off, seg, k, A, B)) continue;
        const JnItem it = jn_classify(A, B, L);
        const int64_t f[JC_FIELDS] = {1, (int64_t)it.kind, it.other, it.past, it.tid, it.x, it.len, it.lo, it.hi, it.tid_hi, it.y, it.o};
        memcpy(o, f, sizeof f);
    }
}

uint64_t fnv(const void *p, size_t bytes) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < bytes; i++) h = (h ^ ((const uint8_t *)p)[i]) * 1099511628211ull;
    return h;
}

Table table_of(int which, uint64_t seed, uint64_t n) { return which ? extreme() : seeded(seed, n); }

}  // namespace

extern "C" {

int jc_fields(void) { return JC_FIELDS; }

// out[n][JC_FIELDS]: record k's junction classified (all zero without a B).
void jc_classify(const int64_t *lim, uint64_t n, const uint64_t *off, const svt_junction_seg *seg, int64_t *out) {
    classify(limits(lim), n, off, seg, out);
}

// Table `which` (0: the seeded one of n records, 1: the extreme-value one): its records and rows, and a copy
// into off[records + 1] / seg[rows].
void jc_table_size(int which, uint64_t seed, uint64_t n, uint64_t *records, uint64_t *rows) {
    const Table t = table_of(which, seed, n);
    *records = t.n();
    *rows = t.seg.size();
}
void jc_table_copy(int which, uint64_t seed, uint64_t n, uint64_t *off, svt_junction_seg *seg) {
    const Table t = table_of(which, seed, n);
    memcpy(off, t.off.data(), t.off.size() * sizeof(uint64_t));
    if (!t.seg.empty()) memcpy(seg, t.seg.data(), t.seg.size() * sizeof(svt_junction_seg));
}

// Both tables classified: one "name digest records" line each and a line of the kinds' counts into out[cap];
// returns the text's length, or -1.
int jc_digest(const int64_t *lim, uint64_t seed, uint64_t n, char *out, int cap) {
    std::string text;
    uint64_t kinds[6] = {0, 0, 0, 0, 0, 0}, junctions = 0, other = 0, past = 0;
    for (int which = 0; which < 2; which++) {
        const Table t = table_of(which, seed, n);
        std::vector<int64_t> r(t.n() * JC_FIELDS);
        classify(limits(lim), t.n(), t.off.data(), t.seg.data(), r.data());
        for (uint64_t k = 0; k < t.n(); k++) {
            const int64_t *o = r.data() + k * JC_FIELDS;
            junctions += (uint64_t)o[0], other += (uint64_t)o[2], past += (uint64_t)o[3];
            if (o[0]) kinds[o[1]]++;
        }
        char line[96];
        snprintf(line, sizeof line, "%s %016llx %llu\n", which ? "extreme" : "seeded", (unsigned long long)fnv(r.data(), r.size() * sizeof(int64_t)),
                 (unsigned long long)t.n());
        text += line;
    }
    char line[256];
    snprintf(line, sizeof line, "junctions %llu none %llu del %llu ins %llu dup %llu inv %llu bnd %llu other %llu past %llu\n",
             (unsigned long long)junctions, (unsigned long long)kinds[0], (unsigned long long)kinds[1], (unsigned long long)kinds[2],
             (unsigned long long)kinds[3], (unsigned long long)kinds[4], (unsigned long long)kinds[5], (unsigned long long)other,
             (unsigned long long)past);
    text += line;
    if ((int)text.size() >= cap) return -1;
    memcpy(out, text.c_str(), text.size() + 1);
    return (int)text.size();
}

}  // extern "C"
