/* bucket_model.c -- TEST INFRASTRUCTURE: a CPU model of the engine's value-bucketed event index
 * (svtrek_amd/csrc/svt_bucket.inc, svt_bucket_build.inc), checked against the oracle
 * (oracle/svtrek_oracle.c) window by window.  It restates the design -- events filed by candidate
 * value in 2^BSH-bp buckets per contig, the band's buckets walked, BELOW from per-bucket prefix
 * maxima of a key, ABOVE from the bounded walks only when the vote needs it -- and votes the band
 * plus the two facts with the oracle's own consensus_pos: any window where that differs from the
 * oracle's full walk is a flaw of the design itself, whatever the GPU code does.  It also prints the
 * work the design implies (events walked per window, how often ABOVE is needed).
 * Input: tests/test_bucket_model.py's dump (pileup, loci, clip bits, params).  Exit 1 on a mismatch. */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include "svtrek_oracle.h"   /* oracle/ (tests/test_bucket_model.py passes -I) */

#define SAT (1u << 30)
#define TRAIL 0xEu
#define LEAD 0xFu
typedef struct { uint32_t x, w, z, a; } Ev;
typedef struct { int32_t type, chrom; uint32_t pos, end; } Locus;
typedef struct { Ev *ev; uint64_t n, cap; } Vec;
static void push(Vec *v, Ev e) { if (v->n == v->cap) { v->cap = v->cap ? v->cap * 2 : 1024; v->ev = realloc(v->ev, v->cap * sizeof(Ev)); } v->ev[v->n++] = e; }

static int BSH = 8;
static void rd(void *p, size_t sz, size_t n, FILE *f) {
    if (fread(p, sz, n, f) != n) { fprintf(stderr, "bucket_model: short read\n"); exit(2); }
}
enum { AS, AE, AI, AL, NA_ };
typedef struct { uint32_t nb; uint64_t *off; int64_t *pm; Ev *ev; } Arr;   /* per contig */
static Arr A[4][64];
static uint32_t maxD[64];

static uint32_t val(int k, const Ev *e) {
    uint32_t op = e->w & 15u;
    if (k == AL) return e->x;
    if (k == AE) return op == LEAD ? e->a + 1u : e->x + (e->w >> 4) + 1u;
    return e->x;
}
static int64_t key(int k, const Ev *e) {
    uint32_t op = e->w & 15u;
    if (k == AS) return op == TRAIL ? (e->x < e->z ? e->x : e->z) : e->z;
    if (k == AE) return op == LEAD ? e->x : e->z;
    if (k == AL) return e->a;
    return e->z;
}

int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "rb");
    if (argc > 2) BSH = atoi(argv[2]);
    int64_t h[4]; rd(h, 8, 4, f);
    int nt = (int)h[0]; int64_t nr = h[1]; uint64_t nops = h[2]; int64_t nl = h[3];
    int64_t *tid_off = malloc((nt + 1) * 8); rd(tid_off, 8, nt + 1, f);
    int32_t *pos = malloc(nr * 4), *endpos = malloc(nr * 4); rd(pos, 4, nr, f); rd(endpos, 4, nr, f);
    uint64_t *coff = malloc((nr + 1) * 8); rd(coff, 8, nr + 1, f);
    uint32_t *cig = malloc(nops * 4 + 4); rd(cig, 4, nops, f);
    Locus *L = malloc(nl * sizeof(Locus)); rd(L, sizeof(Locus), nl, f);
    uint8_t *clip = malloc(nr + 1);
    int have_clip = fread(clip, 1, nr, f) == (size_t)nr;
    orc_params prm = {20000, 10000, 2000, 500, 5, 3};
    if (have_clip) { int32_t pp[6]; if (fread(pp, 4, 6, f) == 6) memcpy(&prm, pp, sizeof pp); }
    fclose(f);
    if (!have_clip) for (int64_t r = 0; r < nr; r++) { uint64_t o = coff[r], n = coff[r + 1] - o; clip[r] = n ? (((cig[o + n - 1] & 15u) == 4u) | (((cig[o] & 15u) == 4u) << 1)) : 0; }
    int bw = prm.consensus_interval_range + (prm.consensus_interval > 0 ? prm.consensus_interval : 0);
    uint64_t nev[3] = {0, 0, 0};
    for (int t = 0; t < nt; t++) {
        Vec V[4] = {{0}};
        int32_t maxe = 0;
        for (int64_t r = tid_off[t]; r < tid_off[t + 1]; r++) {
            uint32_t p = (uint32_t)pos[r], cur = p < SAT ? p : SAT;
            uint32_t n = (uint32_t)(coff[r + 1] - coff[r]);
            const uint32_t *c = cig + coff[r];
            if (endpos[r] > maxe) maxe = endpos[r];
            if (pos[r] > maxe) maxe = pos[r];
            for (uint32_t i = 0; i < n; i++) {
                uint32_t op = c[i] & 15u, len = c[i] >> 4;
                if (op == 2 && len > 50) { Ev e = {cur, c[i], (uint32_t)endpos[r], p}; push(&V[AS], e); push(&V[AE], e); if (len > maxD[t]) maxD[t] = len; }
                if (op == 1 && len >= 50) { Ev e = {cur, c[i], (uint32_t)endpos[r], p}; push(&V[AI], e); }
                uint32_t adv = (op == 1 || op == 4) ? 0 : len;
                cur = cur + adv < SAT && cur + adv >= cur ? cur + adv : SAT;
            }
            if (clip[r] & 1u) { Ev e = {cur, TRAIL, (uint32_t)endpos[r], p}; push(&V[AS], e); }
            if (clip[r] & 2u) { Ev e = {p, LEAD, (uint32_t)endpos[r], cur}; push(&V[AE], e); push(&V[AL], e); }
        }
        uint64_t vc = (uint64_t)maxe + 65536;
        uint32_t nb = (uint32_t)((vc + (1u << BSH) - 1) >> BSH) + 1;   /* last = overflow */
        for (int k = 0; k < 4; k++) {
            Arr *a = &A[k][t];
            a->nb = nb;
            a->off = calloc(nb + 1, 8);
            a->pm = malloc(nb * 8);
            for (uint64_t i = 0; i < V[k].n; i++) { uint32_t b = val(k, &V[k].ev[i]) >> BSH; if (b > nb - 1) b = nb - 1; a->off[b + 1]++; }
            for (uint32_t b = 0; b < nb; b++) a->off[b + 1] += a->off[b];
            uint64_t *cur = malloc(nb * 8); memcpy(cur, a->off, nb * 8);
            a->ev = malloc((V[k].n + 1) * sizeof(Ev));
            for (int b = 0; b < (int)nb; b++) a->pm[b] = -1;
            for (uint64_t i = 0; i < V[k].n; i++) {
                uint32_t b = val(k, &V[k].ev[i]) >> BSH; if (b > nb - 1) b = nb - 1;
                a->ev[cur[b]++] = V[k].ev[i];
                int64_t kk = key(k, &V[k].ev[i]); if (kk > a->pm[b]) a->pm[b] = kk;
            }
            for (uint32_t b = 1; b < nb; b++) if (a->pm[b - 1] > a->pm[b]) a->pm[b] = a->pm[b - 1];
            if (k < 3) nev[k] += V[k].n;
            free(cur); free(V[k].ev);
        }
    }
    fprintf(stderr, "events S %lu E %lu I %lu\n", nev[0], nev[1], nev[2]);
    /* oracle */
    orc_pileup op = {nt, tid_off, pos, endpos, coff, cig, clip};
    orc_result *want = malloc(nl * sizeof(orc_result));
    orc_refine_batch(&op, &prm, (const orc_locus *)L, nl, want, 8, NULL);
    uint64_t win[3] = {0}, band_ev[3] = {0}, above_need[3] = {0}, above_ev[3] = {0}, above_found[3] = {0}, redo[3] = {0},
             bad = 0, lead_ev = 0, lead_found = 0, span_ev = 0, span_found = 0, none_found = 0, below_pm[3] = {0}, below_walk[3] = {0}, vote[3] = {0}, maxband = 0;
    for (int64_t li = 0; li < nl; li++) {
        for (int w = 0; w < 2; w++) {
            Locus l = L[li];
            int k; uint32_t s, e, imp;
            if (l.type == 1 && w == 0) { k = AI; s = l.pos - prm.median_interval; e = l.pos + prm.median_interval; imp = l.pos; }
            else if (l.type == 2 && w == 0) { k = AS; s = l.pos - prm.wider_interval; e = l.pos + prm.narrow_interval; imp = l.pos; }
            else if (l.type == 2) { k = AE; s = l.end - prm.narrow_interval; e = l.end + prm.narrow_interval; imp = l.end; }
            else continue;
            uint32_t got = 0xffffffffu, ref = w ? want[li].end : want[li].start;
            win[k]++;
            int tid = l.chrom - 1;
            int64_t beg = (int64_t)(uint32_t)(s - 1u), qend = (int64_t)(uint32_t)(e - 1u);
            int64_t lo = (int64_t)(int32_t)imp - bw, hi = (int64_t)(int32_t)imp + bw;
            int members[4096]; int nbm = 0; int below = 0, above = 0;
            int band_ok = prm.consensus_interval_range > 25 && bw <= 1023 && prm.consensus_interval >= -1023;
            int sent_ok = (int64_t)prm.narrow_interval + 2 >= (bw > 26 ? bw : 26);
            if (!band_ok || (k == AE && !sent_ok) || (int32_t)imp <= -(1 << 30) || (int32_t)imp >= (1 << 30) || lo < -(1 << 29)) { redo[k]++; continue; }
            if (tid >= 0 && tid < nt && qend > beg && tid_off[tid + 1] > tid_off[tid]) {
                if (lo >= qend || e >= SAT) { redo[k]++; continue; }
                Arr *a = &A[k][tid];
                uint32_t top = a->nb - 1;
                int64_t bl64 = lo < 0 ? 0 : lo >> BSH, bh64 = hi - 1 < 0 ? -1 : (hi - 1) >> BSH;
                uint32_t bL = bl64 > top ? top : (uint32_t)bl64, bH = bh64 > top ? top : (uint32_t)bh64;
                if (bL > 0 && a->pm[bL - 1] > beg) { below = 1; below_pm[k]++; }
                #define CAND(E_, V_, ABOVE_BRK) do { \
                    const Ev *ev_ = (E_); uint32_t op_ = ev_->w & 15u; int c_ = 0; ABOVE_BRK = 0; \
                    if (k == AE && op_ == LEAD) { \
                        uint32_t pr = ev_->x; \
                        if (pr >= s && (int64_t)pr < qend && (int64_t)ev_->z > beg) { if (ev_->a > e) ABOVE_BRK = 1; else c_ = 1; } \
                    } else { \
                        int y_ = (int64_t)ev_->a < qend && (int64_t)ev_->z > beg && ev_->x <= e; \
                        if (k == AS && op_ == TRAIL) c_ = y_ && ev_->x >= s; else c_ = y_; \
                    } \
                    V_ = c_; } while (0)
                if (bh64 >= 0) {
                    for (uint64_t i = a->off[bL]; i < a->off[bH + 1]; i++) {
                        int c, brk; CAND(&a->ev[i], c, brk);
                        band_ev[k]++;
                        if (brk) { above = 1; continue; }
                        if (!c) continue;
                        int64_t v = val(k, &a->ev[i]);
                        if (v <= lo) { if (!below) below_walk[k]++; below = 1; }
                        else if (v >= hi) above = 1;
                        else members[nbm++] = (int)v;
                    }
                }
                if (nbm > (int)maxband) maxband = nbm;
                if (nbm >= prm.consensus_min_count) {
                    int mn = 0x7fffffff; for (int i = 0; i < nbm; i++) if (members[i] < mn) mn = members[i];
                    int lt = below || mn < (int)imp - 25;
                    if (!lt && !above) {
                        above_need[k]++;
                        int64_t eu = k == AE ? (int64_t)e + 1 : (int64_t)e;
                        uint32_t b0 = (uint32_t)((hi >> BSH) > top ? top : (hi >> BSH)), b1 = (uint32_t)((eu >> BSH) > top ? top : (eu >> BSH));
                        for (uint64_t i = a->off[b0]; i < a->off[b1 + 1] && !above; i++) {
                            int c, brk; CAND(&a->ev[i], c, brk); above_ev[k]++;
                            if (brk) { above = 1; break; }
                            if (c && (int64_t)val(k, &a->ev[i]) >= hi) above = 1;
                        }
                        if (above) above_found[k]++;
                        else if (k == AE) {
                            /* (b) breaking LEADs: LEAD events by read start in [s, qend) with walkend > e */
                            Arr *al = &A[AL][tid];
                            uint32_t t2 = al->nb - 1;
                            uint32_t c0 = (uint32_t)(((int64_t)s >> BSH) > t2 ? t2 : ((int64_t)s >> BSH));
                            uint32_t c1 = (uint32_t)(((qend - 1) >> BSH) > t2 ? t2 : ((qend - 1) >> BSH));
                            for (uint64_t i = al->off[c0]; i < al->off[c1 + 1] && !above; i++) {
                                const Ev *ev = &al->ev[i]; lead_ev++;
                                if (ev->x >= s && (int64_t)ev->x < qend && ev->a > e) above = 1;
                            }
                            if (above) lead_found++;
                            else {
                                /* (c) D spanning e: S-array buckets over [e - maxD, e] */
                                Arr *as = &A[AS][tid];
                                uint32_t t3 = as->nb - 1;
                                int64_t xl = (int64_t)e - (int64_t)maxD[tid];
                                if (xl < 0) xl = 0;
                                uint32_t d0 = (uint32_t)((xl >> BSH) > t3 ? t3 : (xl >> BSH)), d1 = (uint32_t)(((int64_t)e >> BSH) > t3 ? t3 : ((int64_t)e >> BSH));
                                for (uint64_t i = as->off[d0]; i < as->off[d1 + 1] && !above; i++) {
                                    const Ev *ev = &as->ev[i]; span_ev++;
                                    if ((ev->w & 15u) != 2u) continue;
                                    if (ev->x <= e && ev->x + (ev->w >> 4) > e && (int64_t)ev->a < qend && (int64_t)ev->z > beg) above = 1;
                                }
                                if (above) span_found++; else none_found++;
                            }
                        }   /* spanning D / breaking LEAD beyond e+1: the exact fallback */
                    }
                }
                vote[k]++;
                int m2[4100]; int n2 = 0;
                for (int i = 0; i < nbm; i++) m2[n2++] = members[i];
                if (below) m2[n2++] = (int)lo;
                if (above) m2[n2++] = (int)hi;
                got = (uint32_t)orc_consensus_pos(m2, n2, (int)imp, prm.consensus_min_count, prm.consensus_interval,
                                                  prm.consensus_interval_range);
                if (nbm < prm.consensus_min_count) got = 0xffffffffu;
            }
            if (got != ref) { if (bad < 10) fprintf(stderr, "MISMATCH locus %ld w %d kind %d got %u want %u nb %d below %d above %d\n", (long)li, w, k, got, ref, nbm, below, above); bad++; }
        }
    }
    const char *kn[3] = {"START", "END", "INS"};
    for (int k = 0; k < 3; k++)
        printf("%-5s windows %8lu band_ev/win %6.2f below_pm %5.3f below_walk %5.3f vote %5.3f above_need %6.4f above_found %6.4f above_ev/need %6.2f redo %6.4f\n",
               kn[k], win[k], (double)band_ev[k] / win[k], (double)below_pm[k] / win[k], (double)below_walk[k] / win[k], (double)vote[k] / win[k],
               (double)above_need[k] / win[k], (double)above_found[k] / win[k], above_need[k] ? (double)above_ev[k] / above_need[k] : 0, (double)redo[k] / win[k]);
    printf("END above: lead_ev %lu lead_found %lu span_ev %lu span_found %lu none %lu maxD %u\n", lead_ev, lead_found, span_ev, span_found, none_found, maxD[0]);
    printf("walked total %lu (built %lu) maxband %lu mismatches %lu\n", band_ev[0] + band_ev[1] + band_ev[2] + above_ev[0] + above_ev[1] + above_ev[2],
           nev[0] + nev[2] + (nev[1] - 0), maxband, bad);
    return bad != 0;
}
