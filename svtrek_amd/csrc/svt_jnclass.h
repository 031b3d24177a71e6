// svt_jnclass.h -- a table record's junction (A, B) and what it stands for, free of HIP: plain C++17, so
// that it compiles with g++ alone for the CPU model test (tests/test_jnclass_model.py) and under the
// sanitizers (tests/san/jnclass_san.cpp) as well as inside the engine, where junction_kernel
// (svt_junction.inc), rearr_kernel (svt_rearr.inc) and bnd_kernel (svt_bnd.inc) call it.  The rows are
// untrusted 32-bit fields; every difference is taken in signed 64 bits.  It defines no thresholds or clamps:
// the engine passes its own in JnLimits.
//
// jn_classify is the only place that knows the rules of include/svtrek_junction.h (DEL / INS),
// svtrek_rearr.h (DUP / INV) and svtrek_bnd.h (BND).  They partition the junctions: one gives at most one
// item, and independently of that counts in svt_call_junction_stats.other or not.
//
//   B.tid != A.tid                   other; BND (no threshold)
//   B.strand != A.strand             other; INV iff |p - q| > min_len: (min(p, q), |p - q|)
//   same contig and strand           (Lf, Rt) = (A, B) on strand +, (B, A) on -;
//                                    dr = Rt.r_beg - Lf.r_end, dq = B.q_beg - A.q_end, d = dr - dq
//     d > min_len and dr > 0         DEL: (Lf.r_end, d)
//     -d >= min_len, dr < -min_len   DUP: (Rt.r_beg, -dr); other iff dq > 0
//     -d >= min_len, dr >= -min_len  INS iff dq > 0: (Lf.r_end, -d)
// with p = A.r_end on strand + / A.r_beg on -, q = B.r_beg on strand + / B.r_end on -.
#ifndef SVT_JNCLASS_H
#define SVT_JNCLASS_H

#include <stdint.h>

#include "../../include/svtrek_junction.h"

#ifdef __HIPCC__
#define JN_FN __host__ __device__ __forceinline__
#else
#define JN_FN inline
#endif

enum JnKind : uint32_t { JN_NONE = 0, JN_DEL, JN_INS, JN_DUP, JN_INV, JN_BND };
constexpr uint32_t JN_ALL = 1u << JN_DEL | 1u << JN_INS | 1u << JN_DUP | 1u << JN_INV | 1u << JN_BND;

struct JnLimits {
    int64_t min_len;      // the length thresholds (50)
    uint32_t x_sat;       // x of a bucketed item saturates here; x (or y, BND) at or past it: `past`
    uint32_t len_max;     // len of a bucketed item is clamped to it
    uint32_t ext_max;     // so are the two extent words
};

// The item as the build kernels file it.  DEL / INS / DUP / INV: contig tid, x saturated, len clamped, the
// extent (lo, hi) = (min r_beg, max r_end) of A and B clamped.  BND: (tid, x, tid_hi, y, o), x and y as
// they are.  Fields a kind does not have are 0.
struct JnItem {
    JnKind kind;
    bool other;           // svt_call_junction_stats.other counts the junction (whatever the kind)
    bool past;            // x >= x_sat (BND: x or y): the scan, or the BND build, drops and counts the item
    int32_t tid, tid_hi;
    uint32_t x, len, lo, hi, y, o;
};

// a < b in the order of the tuple (q_beg, q_end, tid, r_beg, strand)
JN_FN bool jn_less(const svt_junction_seg &a, const svt_junction_seg &b) {
    if (a.q_beg != b.q_beg) return a.q_beg < b.q_beg;
    if (a.q_end != b.q_end) return a.q_end < b.q_end;
    if (a.tid != b.tid) return a.tid < b.tid;
    if (a.r_beg != b.r_beg) return a.r_beg < b.r_beg;
    return a.strand < b.strand;
}

// The junction of table record k (include/svtrek_junction.h): A its first row, B the smallest tuple
// strictly greater than A's among the others, by one pass over the record's rows.  Returns whether
// there is one.  (The loop walks a pointer: the indexed spelling costs the build kernels registers,
// profiles/call_index/README.md.)
JN_FN bool jn_next(const uint64_t *off, const svt_junction_seg *seg, uint64_t k, svt_junction_seg &A, svt_junction_seg &B) {
    const uint64_t r0 = off[k], r1 = off[k + 1];
    A = seg[r0];
    B = A;
    bool have = false;
    for (const svt_junction_seg *p = seg + r0 + 1, *e = seg + r1; p < e; p++) {
        const svt_junction_seg t = *p;
        if (jn_less(A, t) && (!have || jn_less(t, B))) {
            B = t;
            have = true;
        }
    }
    return have;
}

// The junction (A, B) classified.  WANT is the mask (1 << kind) of the kinds the caller files: a kind
// outside it comes back as JN_NONE and its arithmetic is not compiled; `other` is always right.
template <uint32_t WANT = JN_ALL>
JN_FN JnItem jn_classify(const svt_junction_seg &A, const svt_junction_seg &B, const JnLimits &L) {
    constexpr bool del = WANT >> JN_DEL & 1u, ins = WANT >> JN_INS & 1u, dup = WANT >> JN_DUP & 1u, inv = WANT >> JN_INV & 1u,
                   bnd = WANT >> JN_BND & 1u;
    JnItem it{};
    uint32_t x = 0;   // (a row's field, or the smaller of two)
    int64_t len = 0;
    if (B.tid != A.tid || B.strand != A.strand) {
        it.other = true;
        if ((bnd && B.tid != A.tid) || (inv && B.tid == A.tid)) {
            const int64_t p = A.strand ? (int64_t)A.r_beg : (int64_t)A.r_end;
            const int64_t q = B.strand ? (int64_t)B.r_end : (int64_t)B.r_beg;
            if (B.tid != A.tid) {
                const uint32_t sa = A.strand, sb = 1u - B.strand;
                const bool a_lo = A.tid < B.tid;
                it.kind = JN_BND;
                it.tid = a_lo ? A.tid : B.tid;
                it.tid_hi = a_lo ? B.tid : A.tid;
                it.x = (uint32_t)(a_lo ? p : q);
                it.y = (uint32_t)(a_lo ? q : p);
                it.o = a_lo ? 2u * sa + sb : 2u * sb + sa;
                it.past = it.x >= L.x_sat || it.y >= L.x_sat;
                return it;
            }
            const int64_t w = p > q ? p - q : q - p;
            if (w > L.min_len) {
                it.kind = JN_INV;
                x = (uint32_t)(p < q ? p : q);
                len = w;
            }
        }
    } else {
        const svt_junction_seg &Lf = A.strand ? B : A, &Rt = A.strand ? A : B;
        const int64_t dr = (int64_t)Rt.r_beg - (int64_t)Lf.r_end, dq = (int64_t)B.q_beg - (int64_t)A.q_end, d = dr - dq;
        if (d > L.min_len && dr > 0) {
            if (del) it.kind = JN_DEL;
        } else if (-d >= L.min_len) {
            if (dr < -L.min_len) {
                it.other = dq > 0;
                if (dup) it.kind = JN_DUP;
            } else if (ins && dq > 0) {
                it.kind = JN_INS;
            }
        }
        if (it.kind != JN_NONE) {
            x = dup && it.kind == JN_DUP ? Rt.r_beg : Lf.r_end;
            len = dup && it.kind == JN_DUP ? -dr : del && it.kind == JN_DEL ? d : -d;
        }
    }
    if (it.kind != JN_NONE) {
        const uint32_t b0 = A.r_beg < B.r_beg ? A.r_beg : B.r_beg, e1 = A.r_end > B.r_end ? A.r_end : B.r_end;
        it.tid = A.tid;
        it.x = x < L.x_sat ? x : L.x_sat;
        it.len = (uint32_t)(len < (int64_t)L.len_max ? len : (int64_t)L.len_max);
        it.lo = b0 < L.ext_max ? b0 : L.ext_max;
        it.hi = e1 < L.ext_max ? e1 : L.ext_max;
        it.past = it.x >= L.x_sat;
    }
    return it;
}

#endif  // SVT_JNCLASS_H
