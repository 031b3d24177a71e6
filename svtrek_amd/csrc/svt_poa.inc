// svt_poa.inc -- allele-consensus mode (included by svt_engine.hip inside its anonymous
// namespace): banded partial-order alignment (POA) consensus of the inserted sequences that
// support a refined INS call, one wavefront per locus.
//
// The north star names "abPOA banded partial-order consensus"; the reference declares abPOA
// as a submodule (.gitmodules:4-6) but never includes or calls it (Makefile:16), and its
// sources are absent, so there is no reference behaviour: this follows abPOA's published
// design (global POA against the graph in topological order, adaptive band of width
// b + f*len around the predecessors' best cells, fusion of matching bases into the graph,
// heaviest-bundle consensus) with the exact rules of oracle/poa_oracle.c (the checker; parity
// unpinned by the reference).  Integer DP, no MFMA: one band row (<= 128 cells, 2 per lane)
// per graph node, the row's insertion chain as a wave max-scan, rows / backtrack codes /
// graph in a per-wave HBM scratch slot.

constexpr int POA_PIN = 32;             // in-edges per node (each fused sequence adds <= 1)
constexpr int POA_AL = 4;               // aligned alternatives per node (5 bases)
constexpr int POA_BW = 128;             // band cells per row (2 per lane); w <= 63
constexpr int POA_SEQ_MAX = 4096;       // longest sequence (LDS buffer)
constexpr int32_t POA_NEG = -(1 << 29); // unreachable
constexpr int32_t POA_KEYNEG = INT32_MIN / 2;
constexpr uint32_t P_MATCH = 0u, P_INS = 1u, P_DEL = 2u;
constexpr uint32_t POA_NOSPILL = 0xffffffffu;

struct PoaParams {   // svt_poa_params
    int32_t match, mismatch, gap_open, gap_ext, band_b, band_f_permille;
    int32_t max_seqs, max_len, max_nodes, support_radius, max_support;
};

// One scratch slot (arrays sized for node_cap + 2 nodes; spill rows for spill_cap nodes).
struct PoaSlot {
    uint8_t *base, *nin, *nal;
    uint16_t *in_pred, *in_w, *al;   // [node][POA_PIN], [node][POA_PIN], [node][POA_AL]
    uint16_t *ord, *ord2, *anc, *aidx, *newrank, *bp;
    uint16_t *prk;                   // [rank][POA_PIN] predecessor ranks (poa_align)
    uint4 *rrec;                     // [rank] {node | in-edges << 16 | base << 24, ranks of in-edges 0-3}
    uint32_t *runlen, *score;
    int32_t *sH, *sE;                // [spill row][POA_BW]: H / E rows read from beyond the LDS ring
    uint2 *sband;                    // [spill row] {lo | hi << 16, mpos} of that row
    uint32_t *sidx;                  // [node] spill row, or POA_NOSPILL
    uint32_t *nspill;                // spill rows taken
    uint16_t *code;                  // [node][POA_BW]
    uint32_t *path;                  // [max_nodes + max_len + 8]
};

struct PoaArgs {
    DevPileup pile;
    KParams prm;
    PoaParams pp;
    const svt_locus *loci;
    const svt_result *refined;
    uint32_t n;
    const uint64_t *ins_base;   // [n_reads] index of each read's first I >= 50 op
    const uint64_t *ins_off;    // [n_ins + 1]
    const uint8_t *ins_bases;   // nt4 codes
    uint8_t *slots;             // nslot * slot_bytes
    uint64_t slot_bytes;
    int32_t node_cap;           // graph nodes a slot holds (<= max_nodes); larger graphs defer
    int32_t spill_cap;          // spill rows a slot holds; more defer (full-size slots: node_cap + 2)
    uint32_t *queue;            // work counter (zeroed before the launch)
    const uint32_t *list;       // loci to process (n entries), or null: 0 .. n-1
    unsigned long long *diag;   // SVT_POA_DIAG builds: per-phase wall-clock ticks, else null
    int32_t *supg;              // [n][max_support] supporting sequences (poa_support_kernel)
    int32_t *nsupg;             // [n] supporting sequences found; -1: not a refined INS call
    uint32_t *est;              // [n] cost estimate: bases of the sequences that will be fused
    int32_t cap;                // consensus bases per locus
    uint8_t *out;               // [n][cap]
    int4 *res;                  // [n] {len, n_support, n_used, status}
};

__host__ __device__ inline uint64_t poa_round(uint64_t b) { return (b + 255) & ~255ull; }

// Bytes of one slot; poa_slot carves them in this order.
__host__ __device__ inline uint64_t poa_slot_bytes(int32_t node_cap, int32_t spill_cap, int32_t max_len) {
    const uint64_t N = (uint64_t)node_cap + 2;
    return 2 * poa_round((uint64_t)spill_cap * POA_BW * 4) + poa_round((uint64_t)spill_cap * 8) +
           poa_round(N * 4) + poa_round(4) +
           poa_round(N * POA_BW * 2) + 3 * poa_round(N * POA_PIN * 2) + poa_round(N * 16) +
           poa_round(N * POA_AL * 2) + 3 * poa_round(N) + 6 * poa_round(N * 2) + 2 * poa_round(N * 4) +
           poa_round((N + (uint64_t)max_len + 8) * 4);
}

__device__ __forceinline__ PoaSlot poa_slot(const PoaArgs &a, uint32_t s) {
    const uint64_t N = (uint64_t)a.node_cap + 2;
    uint8_t *p = a.slots + (uint64_t)s * a.slot_bytes;
    auto take = [&](uint64_t bytes) { uint8_t *r = p; p += poa_round(bytes); return r; };
    PoaSlot q;
    q.sH = (int32_t *)take((uint64_t)a.spill_cap * POA_BW * 4);
    q.sE = (int32_t *)take((uint64_t)a.spill_cap * POA_BW * 4);
    q.sband = (uint2 *)take((uint64_t)a.spill_cap * 8);
    q.sidx = (uint32_t *)take(N * 4);
    q.nspill = (uint32_t *)take(4);
    q.code = (uint16_t *)take(N * POA_BW * 2);
    q.in_pred = (uint16_t *)take(N * POA_PIN * 2);
    q.in_w = (uint16_t *)take(N * POA_PIN * 2);
    q.al = (uint16_t *)take(N * POA_AL * 2);
    q.prk = (uint16_t *)take(N * POA_PIN * 2);
    q.rrec = (uint4 *)take(N * 16);
    q.base = take(N);
    q.nin = take(N);
    q.nal = take(N);
    q.ord = (uint16_t *)take(N * 2);
    q.ord2 = (uint16_t *)take(N * 2);
    q.anc = (uint16_t *)take(N * 2);
    q.aidx = (uint16_t *)take(N * 2);
    q.newrank = (uint16_t *)take(N * 2);
    q.bp = (uint16_t *)take(N * 2);
    q.runlen = (uint32_t *)take(N * 4);
    q.score = (uint32_t *)take(N * 4);
    q.path = (uint32_t *)take((N + (uint64_t)a.pp.max_len + 8) * 4);
    return q;
}

__device__ __forceinline__ void poa_sync() {   // global-memory hand-off between the lanes of one wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ int32_t wave_max_i(int32_t v) { return rdlane_i(wave_scan_max(v), WAVE - 1); }

// Inclusive wave max-scan for values far below zero (identity POA_KEYNEG).
__device__ __forceinline__ int32_t wave_scan_max_k(int32_t v) {
    v = max(v, dpp_i<0x111, 0xf>(v, POA_KEYNEG));
    v = max(v, dpp_i<0x112, 0xf>(v, POA_KEYNEG));
    v = max(v, dpp_i<0x114, 0xf>(v, POA_KEYNEG));
    v = max(v, dpp_i<0x118, 0xf>(v, POA_KEYNEG));
    v = max(v, dpp_i<0x142, 0xa>(v, POA_KEYNEG));
    v = max(v, dpp_i<0x143, 0xc>(v, POA_KEYNEG));
    return v;
}

// in-edge prev -> x: weight + 1, or a new edge (one lane; x's list belongs to that lane)
__device__ __forceinline__ void poa_add_edge(const PoaSlot &g, uint32_t prev, uint32_t x) {
    const uint32_t n = g.nin[x];
    uint16_t *pr = g.in_pred + (uint64_t)x * POA_PIN, *w = g.in_w + (uint64_t)x * POA_PIN;
    for (uint32_t k = 0; k < n; k++)
        if (pr[k] == prev) { w[k] = (uint16_t)(w[k] + 1); return; }
    if (n < (uint32_t)POA_PIN) { pr[n] = (uint16_t)prev; w[n] = 1; g.nin[x] = (uint8_t)(n + 1); }
}

// The first fused sequence: the chain source -> s[0] -> ... -> s[m-1] -> sink.
__device__ void poa_init_chain(const PoaSlot &g, const uint8_t *s, int m, int &n_nodes, int &nord) {
    const int ln = lane_id();
    for (int k = ln; k < m; k += WAVE) {
        const uint32_t x = 2u + (uint32_t)k;
        g.base[x] = s[k];
        g.nin[x] = 1;
        g.nal[x] = 0;
        g.runlen[x] = 0;
        g.in_pred[(uint64_t)x * POA_PIN] = (uint16_t)(k == 0 ? 0u : x - 1u);
        g.in_w[(uint64_t)x * POA_PIN] = 1;
        g.ord[k + 1] = (uint16_t)x;
        g.newrank[x] = (uint16_t)(k + 1);
    }
    if (ln == 0) {
        g.ord[0] = 0;
        g.ord[m + 1] = 1;
        g.newrank[0] = 0;
        g.newrank[1] = (uint16_t)(m + 1);
        g.nin[0] = 0;
        g.nin[1] = 1;
        g.runlen[0] = 0;
        g.runlen[1] = 0;
        g.in_pred[(uint64_t)1 * POA_PIN] = (uint16_t)(m + 1);
        g.in_w[(uint64_t)1 * POA_PIN] = 1;
    }
    n_nodes = m + 2;
    nord = m + 2;
    poa_sync();
}

#ifndef SVT_POA_DIAG
#define SVT_POA_DIAG 0   // 1: per-phase wall-clock accounting into PoaArgs::diag (diagnostic builds)
#endif
enum { PD_SUPPORT, PD_LOAD, PD_ROWS, PD_TRACE, PD_FUSE, PD_CONS, PD_NROWS, PD_NSTEPS, PD_NSEQ, PD_NFAR,
        PD_T0, PD_T1, PD_LOCMAX, PD_WAVEMAX, PD_N };
__device__ __forceinline__ void pdiag(unsigned long long *d, int k, unsigned long long &t) {
    if (SVT_POA_DIAG && d) {
        const unsigned long long now = wall_clock64();
        if (lane_id() == 0) atomicAdd(d + k, now - t);
        t = now;
    }
}
__device__ __forceinline__ void pcount(unsigned long long *d, int k, unsigned long long v) {
    if (SVT_POA_DIAG && d && lane_id() == 0) atomicAdd(d + k, v);
}

// LDS ring of the last POA_RING band rows (by rank): H, E and {lo, hi, mpos}.  Nearly every
// predecessor of a row lies within a few ranks of it (the graph is a chain with short
// bubbles), so the per-row critical path runs in LDS; rows also go to the slot in HBM (the
// traceback's codes, and H/E for the rare predecessor further back than the ring).
#ifndef SVT_POA_RING
#define SVT_POA_RING 8    // test builds shrink it to drive the spill path (tests/test_gpu_poa.py)
#endif
constexpr int POA_RING = SVT_POA_RING;
struct PoaRing {
    int32_t H[POA_RING][POA_BW];
    int32_t E[POA_RING][POA_BW];
    uint32_t lohi[POA_RING];   // lo | hi << 16
    int32_t mpos[POA_RING];
    uint4 rows[2][WAVE];       // staged row records (rrec) of the current and next 64 ranks
};

__device__ __forceinline__ void vm_wait() { __builtin_amdgcn_s_waitcnt(0x0F70); }   // vmcnt(0)
// A load the compiler must keep a global_load: next to an LDS read of the same shape it would
// otherwise merge both into a flat_load, whose wait also drains this wave's HBM stores.
template <typename T>
__device__ __forceinline__ T gld(const T *p) {
    return *(const __attribute__((address_space(1))) T *)p;
}
__device__ __forceinline__ uint2 gld(const uint2 *p) {
    const unsigned long long x = gld(reinterpret_cast<const unsigned long long *>(p));
    return make_uint2((uint32_t)x, (uint32_t)(x >> 32));
}
// Order LDS accesses across lanes of one wave: the hardware executes a wave's LDS operations
// in issue order, so only the compiler must not move them across this point (no lgkmcnt drain).
__device__ __forceinline__ void lds_order() { asm volatile("" ::: "memory"); }

__device__ __forceinline__ void lds_sync() {   // LDS hand-off between the lanes of one wave (no HBM wait)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Align s (LDS, length m) to the graph; writes the path backwards to g.path and returns its
// length, -1 when no sink predecessor's band reaches column m, or -2 when the rows read from
// beyond the ring outnumber the slot's spill rows (the locus defers).  Band cells are stored
// by column: cell j of a row at [j & (POA_BW - 1)] (a band spans <= 127 columns).
// Traceback from (ub, m), the path stored backwards in g.path (kind << 30 | node << 12 |
// sequence index); returns its length.  The walk is a pointer chase, so it runs on a window of
// W ranks staged in LDS (the ring's H/E bytes, free once the rows are done): the code rows of
// ranks (top - W, top] and, in lane top - rank, that node's first two in-edges and their
// ranks.  A refill is three HBM round trips for up to W ranks of path; a step is one LDS read.
__device__ int poa_traceback(const PoaSlot &g, PoaRing &rg, uint32_t ub, int m) {
    constexpr int W = (int)(sizeof(rg.H) + sizeof(rg.E)) / (POA_BW * 2);
    static_assert(W >= 1 && W <= WAVE, "traceback window");
    constexpr int CM = POA_BW - 1;
    const uint16_t *wc = reinterpret_cast<const uint16_t *>(&rg.H[0][0]);
    uint32_t *wc32 = reinterpret_cast<uint32_t *>(&rg.H[0][0]);
    const uint32_t *code32 = reinterpret_cast<const uint32_t *>(g.code);
    const int ln = lane_id();
    uint32_t w_pr = 0, w_rk = 0;   // lane k: first two in-edges of rank top - k, and their ranks
    int top = -1;
    auto refill = [&](int rtop) {
        top = rtop;
        const int rk = rtop - ln;
        const bool ok = ln < W && rk >= 1;   // rank 0 is the source: it has no row
        uint32_t node = 0, pr = 0, np = 0;
        if (ok) node = g.ord[rk];
        if (ok) {
            np = g.nin[node];
            pr = *reinterpret_cast<const uint32_t *>(g.in_pred + (uint64_t)node * POA_PIN);
        }
        uint32_t cw[W];
#pragma unroll
        for (int k = 0; k < W; k++) {   // the code row of window slot k: 64 lanes x 4 bytes
            const uint32_t nk = rdlane(node, k);
            cw[k] = rtop - k >= 1 ? code32[(uint64_t)nk * (POA_BW / 2) + ln] : 0u;
        }
        uint32_t rr = 0;
        if (ok) {
            rr = g.newrank[pr & 0xffffu];
            if (np >= 2) rr |= (uint32_t)g.newrank[pr >> 16] << 16;
        }
        lds_order();
#pragma unroll
        for (int k = 0; k < W; k++) wc32[k * (POA_BW / 2) + ln] = cw[k];
        lds_order();
        w_pr = pr;
        w_rk = rr;
    };
    uint32_t v = ub;
    int vr = uniform_i((int32_t)g.newrank[ub]);
    int jj = m, state = 0, n = 0;
    auto emit = [&](uint32_t x) {
        if (ln == 0) g.path[n] = x;
        n++;
    };
    for (;;) {
        if (v == 0) {
            for (int q = jj; q >= 1; q--) emit(P_INS << 30 | (uint32_t)(q - 1));
            break;
        }
        if (vr > top || vr <= top - W) refill(vr);
        const int slot = top - vr;
        const uint32_t cd = (uint32_t)uniform_i((int32_t)wc[slot * POA_BW + (jj & CM)]);
        auto pred = [&](uint32_t k) {
            if (k < 2) {
                v = (rdlane(w_pr, slot) >> (16 * k)) & 0xffffu;
                vr = (int)((rdlane(w_rk, slot) >> (16 * k)) & 0xffffu);
            } else {   // in-edges past the second: from HBM
                v = (uint32_t)uniform_i((int32_t)g.in_pred[(uint64_t)v * POA_PIN + k]);
                vr = uniform_i((int32_t)g.newrank[v]);
            }
        };
        if (state == 0) {
            const int sr = (int)(cd & 3u);
            if (sr == 0) {
                emit(P_MATCH << 30 | v << 12 | (uint32_t)(jj - 1));
                pred((cd >> 4) & 63u);
                jj -= 1;
            } else {
                state = sr;
            }
        } else if (state == 1) {
            emit(P_DEL << 30 | v << 12);
            state = ((cd >> 2) & 1u) ? 1 : 0;
            pred((cd >> 10) & 63u);
        } else {
            emit(P_INS << 30 | (uint32_t)(jj - 1));
            state = ((cd >> 3) & 1u) ? 2 : 0;
            jj -= 1;
        }
    }
    return n;
}

// Q band cells per lane: 1 when the band (2w + 1 columns) fits the wave, else 2.
template <int Q>
__device__ int poa_align_q(const PoaSlot &g, PoaRing &rg, const PoaParams &pp, const uint8_t *s, int m, int nord,
                           int spill_cap, unsigned long long *dg) {
    unsigned long long t0 = SVT_POA_DIAG ? wall_clock64() : 0ull;
    const int ln = lane_id();
    const int32_t O = pp.gap_open, E = pp.gap_ext;
    constexpr int CM = POA_BW - 1;
    const int w = pp.band_b + (int)((int64_t)pp.band_f_permille * m / 1000);
    // Pre-pass (the order is fixed during the alignment): each row's record and predecessor
    // ranks; a predecessor more than POA_RING ranks back (the sink's included) gets a spill row.
    for (int x = ln; x < nord; x += WAVE) g.sidx[x] = POA_NOSPILL;
    if (ln == 0) *g.nspill = 0;
    poa_sync();
    for (int r = 1 + ln; r < nord; r += WAVE) {
        const uint32_t v = g.ord[r];
        const int np = g.nin[v];
        uint32_t pk[4] = {0, 0, 0, 0};
        for (int k = 0; k < np; k++) {
            const uint32_t u = g.in_pred[(uint64_t)v * POA_PIN + k];
            const uint32_t x = g.newrank[u];
            g.prk[(uint64_t)r * POA_PIN + k] = (uint16_t)x;
            if (k < 4) pk[k] = x;
            if (r - (int)x > POA_RING && atomicCAS(&g.sidx[u], POA_NOSPILL, POA_NOSPILL - 1u) == POA_NOSPILL)
                g.sidx[u] = atomicAdd(g.nspill, 1u);
        }
        g.rrec[r] = make_uint4(v | (uint32_t)np << 16 | (uint32_t)g.base[v] << 24, pk[0] | pk[1] << 16,
                               pk[2] | pk[3] << 16, 0u);
    }
    poa_sync();
    if ((int)rdlane(*g.nspill, 0) > spill_cap) return -2;
    for (int r = 1 + ln; r < nord; r += WAVE) g.rrec[r].w = g.sidx[g.ord[r]];
    {   // source row: H[0][j] = -(O + E j), no deletion state
        const int hi0 = min(m, w);
        const uint32_t sp = g.sidx[0];
        for (int t = ln; t <= hi0; t += WAVE) {
            const int32_t h = t == 0 ? 0 : -(O + E * t);
            rg.H[0][t] = h;
            rg.E[0][t] = POA_NEG;
            if (sp != POA_NOSPILL) {
                g.sH[(uint64_t)sp * POA_BW + t] = h;
                g.sE[(uint64_t)sp * POA_BW + t] = POA_NEG;
            }
        }
        if (ln == 0) {
            if (sp != POA_NOSPILL) g.sband[sp] = make_uint2((uint32_t)hi0 << 16, 0u);
            rg.lohi[0] = (uint32_t)hi0 << 16;
            rg.mpos[0] = 0;
        }
    }
    poa_sync();
    // Row records reach LDS 64 ranks at a time (one HBM wait per batch, none per row: the
    // per-row path below waits on HBM only in its rare branches, each with its own vm_wait).
    auto stage = [&](int b) {
        const int r = b * WAVE + ln;
        const uint4 q = r < nord ? g.rrec[r] : make_uint4(1u, 0u, 0u, POA_NOSPILL);
        rg.rows[b & 1][ln] = q;
    };
    stage(0);
    stage(1);
    lds_sync();
    uint32_t nfar = 0;
    int32_t r_prev = 0, lo_prev = 0, hi_prev = min(m, w), mpos_prev = 0;   // the last row computed
    // row r + 1's record is read while row r runs (off the row-to-row critical path): its batch
    // is always staged by then (batch b + 1 is staged when batch b starts, into the other buffer)
    uint4 rec_next = rg.rows[0][1];
    for (int r = 1; r < nord; r++) {
        if ((r & (WAVE - 1)) == 0) {   // batch r / 64 starts: stage the next one
            stage((r >> 6) + 1);
            lds_sync();
        }
        const uint4 rec = make_uint4((uint32_t)uniform_i((int32_t)rec_next.x), (uint32_t)uniform_i((int32_t)rec_next.y),
                                     (uint32_t)uniform_i((int32_t)rec_next.z), (uint32_t)uniform_i((int32_t)rec_next.w));
        rec_next = rg.rows[((r + 1) >> 6) & 1][(r + 1) & (WAVE - 1)];
        const uint32_t v = rec.x & 0xffffu;
        const int np = (int)((rec.x >> 16) & 0xffu);
        const uint8_t bv = (uint8_t)(rec.x >> 24);
        if (v == 1) continue;   // the sink has no row
        int32_t D[Q], G[Q], dp[Q], ep[Q], ee[Q], sc[Q];
        int j[Q];
        bool val[Q];
        int lo, hi;
        auto band = [&](int c) {   // the row's band around the predecessors' best column
            lo = max(0, c - w);
            hi = min(m, c + w);
#pragma unroll
            for (int q = 0; q < Q; q++) {
                j[q] = lo + Q * ln + q;
                val[q] = j[q] <= hi;
                D[q] = POA_NEG; G[q] = POA_NEG; dp[q] = 0; ep[q] = 0; ee[q] = 0;
                const uint8_t sb = s[j[q] >= 1 && j[q] <= m ? j[q] - 1 : 0];
                sc[q] = (bv == sb && bv < 4) ? pp.match : -pp.mismatch;
            }
        };
        // in-edge k's contribution: its row [ulo, uhi] in ring slot `slot` (nk) or spill row sp
        // (every index is inside the 128-cell row, so the reads are unconditional and the
        // band tests select: no divergent branches in the row)
        auto acc = [&](int k, int32_t ulo, int32_t uhi, bool nk, int slot, uint64_t sp) {
            int32_t hm[Q], hd[Q], ed[Q];
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const int cm1 = (j[q] - 1) & CM, c0 = j[q] & CM;
                if (nk) {
                    hm[q] = rg.H[slot][cm1]; hd[q] = rg.H[slot][c0]; ed[q] = rg.E[slot][c0];
                } else {
                    hm[q] = gld(g.sH + sp + cm1); hd[q] = gld(g.sH + sp + c0); ed[q] = gld(g.sE + sp + c0);
                }
            }
            if (!nk) vm_wait();
            // all three reads of a cell in one round trip: without this the compiler sinks the
            // deletion reads into the band-test branch and waits on LDS twice per row
#pragma unroll
            for (int q = 0; q < Q; q++) asm volatile("" : "+v"(hm[q]), "+v"(hd[q]), "+v"(ed[q]));
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const int jj = j[q];
                const bool okm = val[q] && jj >= 1 && jj - 1 >= ulo && jj - 1 <= uhi && hm[q] > POA_NEG;
                const bool okd = val[q] && jj >= ulo && jj <= uhi;
                const int32_t cand = hm[q] + sc[q];   // match / mismatch from u
                if (okm && cand > D[q]) { D[q] = cand; dp[q] = k; }
                const int32_t aa = hd[q] <= POA_NEG ? POA_NEG : hd[q] - O - E;   // node v deleted, from u
                const int32_t bb = ed[q] <= POA_NEG ? POA_NEG : ed[q] - E;
                const int32_t vv = bb > aa ? bb : aa;
                if (okd && vv > G[q]) { G[q] = vv; ep[q] = k; ee[q] = bb > aa; }
            }
        };
        const int32_t rk0 = (int32_t)(rec.y & 0xffffu);
        if (np == 1 && r - rk0 <= POA_RING) {   // one in-edge, its row in the ring: the common row
            int32_t ulo = lo_prev, uhi = hi_prev, upm = mpos_prev;
            if (rk0 != r_prev) {
                const uint32_t lh = rg.lohi[rk0 % POA_RING];
                ulo = (int32_t)(lh & 0xffffu); uhi = (int32_t)(lh >> 16);
                upm = rg.mpos[rk0 % POA_RING];
            }
            band(upm + 1);
            acc(0, ulo, uhi, true, rk0 % POA_RING, 0);
        } else {
            const uint32_t pw = ln < 2 ? rec.y : rec.z;
            int32_t rk = ln < np ? (int32_t)((pw >> ((ln & 1) * 16)) & 0xffffu) : r;
            if (np > 4) {   // in-edges past the fourth: ranks from HBM
                int32_t x = rk;
                if (ln >= 4 && ln < np) x = g.prk[(uint64_t)r * POA_PIN + ln];
                vm_wait();
                rk = x;
            }
            const bool near = r - rk <= POA_RING;
            const bool has = ln < np;
            uint32_t psp = 0;
            int32_t plo = 0, phi = -1, pm = -1;
            if (ballot(has && !near)) {   // a predecessor older than the ring: its spilled row
                nfar++;
                poa_sync();
                if (has && !near) {
                    const uint32_t pu = gld(g.ord + rk);
                    psp = gld(g.sidx + pu);
                    const uint2 b = gld(g.sband + psp);
                    plo = (int32_t)(b.x & 0xffffu); phi = (int32_t)(b.x >> 16); pm = (int32_t)b.y;
                }
                vm_wait();
            }
            if (has && near) {
                if (rk == r_prev) {   // the previous row: its band is in registers
                    plo = lo_prev; phi = hi_prev; pm = mpos_prev;
                } else {
                    const uint32_t lh = rg.lohi[rk % POA_RING];
                    plo = (int32_t)(lh & 0xffffu); phi = (int32_t)(lh >> 16);
                    pm = rg.mpos[rk % POA_RING];
                }
            }
            band(wave_max_i(pm) + 1);
            for (int k = 0; k < np; k++) {
                const int32_t rkk = rdlane_i(rk, k);
                acc(k, rdlane_i(plo, k), rdlane_i(phi, k), r - rkk <= POA_RING, rkk % POA_RING,
                    (uint64_t)rdlane(psp, k) * POA_BW);
            }
        }
        // insertion chain F[j] = max over band cells k < j of max(D,G)[k] - O - E (j - k):
        // an exclusive max-scan of max(D,G)[k] - O + E k, minus E j
        int32_t key[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const int32_t hp = max(D[q], G[q]);
            key[q] = val[q] && hp > POA_NEG ? hp - O + E * j[q] : POA_KEYNEG;
        }
        const int32_t incl = wave_scan_max_k(Q == 2 ? max(key[0], key[Q - 1]) : key[0]);
        const int32_t excl = dpp_i<0x138, 0xf>(incl, POA_KEYNEG);   // wave_shr:1
        int32_t ex[Q];
        ex[0] = excl;
        if (Q == 2) ex[Q - 1] = max(excl, key[0]);
        int32_t F[Q], Hh[Q], src[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) {
            F[q] = ex[q] > POA_KEYNEG ? ex[q] - E * j[q] : POA_NEG;
            if (F[q] < POA_NEG) F[q] = POA_NEG;
            Hh[q] = D[q]; src[q] = 0;
            if (G[q] > Hh[q]) { Hh[q] = G[q]; src[q] = 1; }
            if (F[q] > Hh[q]) { Hh[q] = F[q]; src[q] = 2; }
            if (Hh[q] < POA_NEG) Hh[q] = POA_NEG;
        }
        // fext: F[j] extends F[j-1] (b > a, a = H[j-1]-O-E, b = F[j-1]-E); none at j == lo
        int32_t prevH[Q], prevF[Q];
        prevH[0] = dpp_i<0x138, 0xf>(Hh[Q - 1], POA_NEG);
        prevF[0] = dpp_i<0x138, 0xf>(F[Q - 1], POA_NEG);
        if (Q == 2) { prevH[Q - 1] = Hh[0]; prevF[Q - 1] = F[0]; }
        int32_t best = POA_KEYNEG;
        int bj = 1 << 20;
        const int rs = r % POA_RING;
        const uint32_t vsp = rec.w;
#pragma unroll
        for (int q = 0; q < Q; q++) {
            int fx = 0;
            if (val[q] && j[q] - 1 >= lo) {
                const int32_t aa = prevH[q] <= POA_NEG ? POA_NEG : prevH[q] - O - E;
                const int32_t bb = prevF[q] <= POA_NEG ? POA_NEG : prevF[q] - E;
                fx = bb > aa;
            }
            // the lanes' cells are distinct mod 128, so cells past hi are written too (never read)
            const int t = j[q] & CM;
            const int32_t ev = G[q] < POA_NEG ? POA_NEG : G[q];
            rg.H[rs][t] = Hh[q];
            rg.E[rs][t] = ev;
            if (vsp != POA_NOSPILL) {
                g.sH[(uint64_t)vsp * POA_BW + t] = Hh[q];
                g.sE[(uint64_t)vsp * POA_BW + t] = ev;
            }
            g.code[(uint64_t)v * POA_BW + t] =
                (uint16_t)(src[q] | (ee[q] << 2) | (fx << 3) | (dp[q] << 4) | (ep[q] << 10));
            if (val[q] && Hh[q] > best) { best = Hh[q]; bj = j[q]; }
        }
        // mpos: the smallest column holding the row maximum
        const int32_t bm = wave_max_i(best);
        const int bl = (int)__builtin_ctzll(ballot(best == bm));
        const int mposv = rdlane_i(bj, bl);
        if (ln == 0) {
            if (vsp != POA_NOSPILL) g.sband[vsp] = make_uint2((uint32_t)lo | (uint32_t)hi << 16, (uint32_t)mposv);
            rg.lohi[rs] = (uint32_t)lo | (uint32_t)hi << 16;
            rg.mpos[rs] = mposv;
        }
        r_prev = r; lo_prev = lo; hi_prev = hi; mpos_prev = mposv;
        // the next record is consumed here, at the row's end (else the compiler moves it to
        // scalar registers right after its read, waiting on it at the row's start)
        asm volatile("" : "+v"(rec_next.x), "+v"(rec_next.y), "+v"(rec_next.z), "+v"(rec_next.w));
        lds_order();
    }
    poa_sync();
    pdiag(dg, PD_ROWS, t0);
    pcount(dg, PD_NROWS, (unsigned long long)nord);
    pcount(dg, PD_NFAR, (unsigned long long)nfar);
    // end: the first sink predecessor with column m in its band and the largest H there (the
    // sink is the last rank: its predecessors' rows are in the ring or spilled)
    int ub = -1;
    if (ln == 0) {
        int32_t bs = POA_NEG;
        const int ns = g.nin[1];
        for (int k = 0; k < ns; k++) {
            const uint32_t u = g.in_pred[(uint64_t)1 * POA_PIN + k];
            const int rku = g.newrank[u];
            const bool nk = (nord - 1) - rku <= POA_RING;
            const uint32_t sp = nk ? 0u : g.sidx[u];
            const uint32_t lh = nk ? rg.lohi[rku % POA_RING] : gld(g.sband + sp).x;
            const int ulo = (int)(lh & 0xffffu), uhi = (int)(lh >> 16);
            if (m < ulo || m > uhi) continue;
            const int32_t hv = nk ? rg.H[rku % POA_RING][m & CM] : gld(g.sH + (uint64_t)sp * POA_BW + (m & CM));
            if (hv <= POA_NEG) continue;
            if (ub < 0 || hv > bs) { bs = hv; ub = (int)u; }
        }
    }
    ub = rdlane_i(ub, 0);
    if (ub < 0) return -1;
    const int n = poa_traceback(g, rg, (uint32_t)ub, m);
    poa_sync();
    pdiag(dg, PD_TRACE, t0);
    pcount(dg, PD_NSTEPS, (unsigned long long)n);
    return n;
}

__device__ int poa_align(const PoaSlot &g, PoaRing &rg, const PoaParams &pp, const uint8_t *s, int m, int nord,
                         int spill_cap, unsigned long long *dg = nullptr) {
    const int w = pp.band_b + (int)((int64_t)pp.band_f_permille * m / 1000);
    return 2 * w + 1 <= WAVE ? poa_align_q<1>(g, rg, pp, s, m, nord, spill_cap, dg)
                             : poa_align_q<2>(g, rg, pp, s, m, nord, spill_cap, dg);
}

// The member of y's aligned group (y included) with the largest rank (g.newrank holds the
// ranks of the current order): the group's block end (groups stay contiguous in the order).
__device__ __forceinline__ uint32_t poa_block_end(const PoaSlot &g, uint32_t y) {
    uint32_t e = y, re = g.newrank[y];
    const int na = g.nal[y];
    for (int q = 0; q < na; q++) {
        const uint32_t z = g.al[(uint64_t)y * POA_AL + q];
        const uint32_t rz = g.newrank[z];
        if (rz > re) { re = rz; e = z; }
    }
    return e;
}

// Fuse the aligned sequence into the graph (path steps in parallel, 64 at a time: a path
// visits every node at most once, so the steps touch disjoint in-edge lists and aligned
// groups), then rebuild the topological order as oracle/poa_oracle.c fuse() does: new nodes
// form chains placed right after an anchor -- a mismatch node starts a chain at its aligned
// group's block end, an insertion node extends the chain of the new node before it or starts
// one at the block end of the existing node before it (the source for a leading insertion).
__device__ void poa_fuse(const PoaSlot &g, const uint8_t *s, int n, int &n_nodes, int &nord) {
    const int ln = lane_id();
    const int first_new = n_nodes;
    uint32_t prev_carry = 0;     // last non-deletion node before this chunk
    uint32_t anchor_carry = 0;   // anchor of the chain the next leading insertion joins
    uint32_t count_carry = 0;    // nodes already in that chain
    for (int c0 = 0; c0 < n; c0 += WAVE) {
        const int k = c0 + ln;
        const bool ok = k < n;
        const uint32_t st = ok ? g.path[n - 1 - k] : (P_DEL << 30);
        const uint32_t kind = st >> 30, v = (st >> 12) & 0xffffu, jj = st & 0xfffu;
        int32_t x = -1;
        bool isnew = false;
        uint8_t b = 0;
        if (ok && kind == P_MATCH) {
            b = s[jj];
            if (g.base[v] == b) x = (int32_t)v;
            else {
                const int na = g.nal[v];
                for (int q = 0; q < na; q++) {
                    const uint32_t y = g.al[(uint64_t)v * POA_AL + q];
                    if (g.base[y] == b) { x = (int32_t)y; break; }
                }
                isnew = x < 0;
            }
        } else if (ok && kind == P_INS) {
            b = s[jj];
            isnew = true;
        }
        const bool is_mm = isnew && kind == P_MATCH;
        const bool exist = x >= 0 && !isnew;
        // chain boundaries (existing nodes, mismatch nodes) and their anchors, old ranks
        const bool bnd = exist || is_mm;
        const uint32_t lane_anchor = exist ? poa_block_end(g, (uint32_t)x) : (is_mm ? poa_block_end(g, v) : 0u);
        const uint64_t nm = ballot(isnew);
        if (isnew) {
            x = n_nodes + (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(nm >> 32),
                                                             __builtin_amdgcn_mbcnt_lo((uint32_t)nm, 0u));
            g.base[x] = b;
            g.nin[x] = 0;
            g.nal[x] = 0;
            g.runlen[x] = 0;
        }
        n_nodes += (int)__popcll(nm);
        poa_sync();
        if (is_mm) {   // x joins v's aligned group
            uint32_t mem[POA_AL + 1];
            const int na = g.nal[v];
            mem[0] = v;
            for (int q = 0; q < na; q++) mem[q + 1] = g.al[(uint64_t)v * POA_AL + q];
            int nx = 0;
            for (int q = 0; q <= na; q++) {
                const uint32_t y = mem[q];
                const int ny = g.nal[y];
                if (ny < POA_AL) { g.al[(uint64_t)y * POA_AL + ny] = (uint16_t)x; g.nal[y] = (uint8_t)(ny + 1); }
                if (nx < POA_AL) g.al[(uint64_t)x * POA_AL + nx++] = (uint16_t)y;
            }
            g.nal[x] = (uint8_t)nx;
        }
        // previous non-deletion node of each step
        const bool has = x >= 0;
        const int32_t hl = wave_scan_max(has ? ln : -1);
        const int32_t hx = dpp_i<0x138, 0xf>(hl, -1);                   // last has-lane before me
        const uint32_t xp = (uint32_t)__shfl(x, hx < 0 ? 0 : hx, WAVE);
        const uint32_t prev = hx < 0 ? prev_carry : xp;
        poa_sync();
        if (has) poa_add_edge(g, prev, (uint32_t)x);
        // chains: an insertion joins the chain after the last boundary before it
        const int32_t bl = wave_scan_max(bnd ? ln : -1);                // last boundary lane <= me
        const uint32_t banc = (uint32_t)__shfl((int)lane_anchor, bl < 0 ? 0 : bl, WAVE);
        const bool bmm = __shfl((int)is_mm, bl < 0 ? 0 : bl, WAVE) != 0;
        const uint64_t upto = ln == WAVE - 1 ? ~0ull : ((2ull << ln) - 1ull);
        const uint64_t after = bl < 0 ? ~0ull : (bl == WAVE - 1 ? 0ull : ~((2ull << bl) - 1ull));
        const uint32_t since = (uint32_t)__popcll(nm & upto & after);   // new nodes in (bl, me]
        uint32_t anchor = 0, cidx = 0;
        if (is_mm) {
            anchor = lane_anchor;
            cidx = 0;
        } else if (isnew) {
            anchor = bl < 0 ? anchor_carry : banc;
            cidx = bl < 0 ? count_carry + since - 1u : since - 1u + (bmm ? 1u : 0u);
        }
        if (isnew) {
            g.anc[x] = (uint16_t)anchor;
            g.aidx[x] = (uint16_t)cidx;
            atomicAdd(&g.runlen[anchor], 1u);
        }
        const int32_t lastx = rdlane_i(hl, WAVE - 1);
        if (lastx >= 0) prev_carry = (uint32_t)rdlane_i(x, lastx);
        const int32_t lastb = rdlane_i(bl, WAVE - 1);
        if (lastb >= 0) {
            anchor_carry = rdlane(lane_anchor, lastb);
            const uint64_t tail = lastb == WAVE - 1 ? 0ull : ~((2ull << lastb) - 1ull);
            count_carry = (rdlane((uint32_t)is_mm, lastb) ? 1u : 0u) + (uint32_t)__popcll(nm & tail);
        } else {
            count_carry += (uint32_t)__popcll(nm);
        }
        poa_sync();
    }
    if (ln == 0) poa_add_edge(g, prev_carry, 1u);
    poa_sync();
    // old node at rank r moves to r + (chain nodes anchored at ranks < r); its chain follows it
    uint32_t carry = 0;
    for (int r0 = 0; r0 < nord; r0 += WAVE) {
        const int r = r0 + ln;
        const uint32_t y = r < nord ? g.ord[r] : 0u;
        const uint32_t rl = r < nord ? g.runlen[y] : 0u;
        const uint32_t incl = wave_scan_add(rl);
        const uint32_t nr = (uint32_t)r + carry + incl - rl;
        if (r < nord) {
            g.ord2[nr] = (uint16_t)y;
            g.newrank[y] = (uint16_t)nr;
            g.runlen[y] = 0;
        }
        carry += rdlane(incl, WAVE - 1);
    }
    poa_sync();
    for (int x = first_new + ln; x < n_nodes; x += WAVE) {
        const uint32_t r = g.newrank[g.anc[x]] + 1u + g.aidx[x];
        g.ord2[r] = (uint16_t)x;
        g.newrank[x] = (uint16_t)r;
    }
    nord = n_nodes;
    poa_sync();
    for (int r = ln; r < nord; r += WAVE) g.ord[r] = g.ord2[r];
    poa_sync();
}

// Heaviest bundle: per node (in order) the in-edge with the largest (weight, score of its
// tail), first on ties; the consensus follows the choices back from the sink.
__device__ int poa_consensus_bases(const PoaSlot &g, int nord, uint8_t *out, int cap) {
    const int ln = lane_id();
    if (ln == 0) g.score[0] = 0;
    poa_sync();
    for (int r = 1; r < nord; r++) {
        const uint32_t v = g.ord[r];
        const int np = g.nin[v];
        const uint32_t u = ln < np ? g.in_pred[(uint64_t)v * POA_PIN + ln] : 0u;
        const uint32_t wt = ln < np ? g.in_w[(uint64_t)v * POA_PIN + ln] : 0u;
        const uint32_t su = ln < np ? g.score[u] : 0u;
        const uint64_t key = ln < np ? ((uint64_t)wt << 32 | su) : 0ull;
        uint64_t mx = key;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) { const uint64_t o = __shfl_xor(mx, d, WAVE); mx = o > mx ? o : mx; }
        const uint64_t hit = ballot(ln < np && key == mx);
        const int kb = hit ? __builtin_ctzll(hit) : 0;
        if (ln == kb) {
            g.bp[v] = (uint16_t)(np ? u : 0u);
            g.score[v] = np ? wt + su : 0u;
        }
        poa_sync();
    }
    int len = 0;
    if (ln == 0) {
        for (uint32_t v = g.bp[1]; v >= 2; v = g.bp[v]) g.path[len++] = g.base[v];   // reversed
        for (int k = 0; k < len && k < cap; k++) out[k] = (uint8_t)g.path[len - 1 - k];
    }
    return rdlane_i(len, 0);
}

// Supporting I ops of an INS call refined to R (oracle orc_poa_support): the I >= 50 ops of
// the reads refine_ins's region query yields (refinement.c:290-293), processed by its walk
// (refinement.c:299-316), |position - R| <= support_radius, length <= max_len, in read then
// op order.  Writes sup[0 .. min(n, max_support)) and returns n.
__device__ int poa_support(const PoaArgs &a, int32_t *sup, int chrom, uint32_t s, uint32_t e, uint32_t R) {
    const DevPileup &P = a.pile;
    const int ln = lane_id();
    const int64_t beg = (int64_t)(uint32_t)(s - 1u), end = (int64_t)(uint32_t)(e - 1u);
    int64_t lo, hi;
    if (!read_range(P, chrom - 1, beg, end, lo, hi)) return 0;
    int nsel = 0;
    for (int64_t rb = lo; rb < hi; rb += WAVE) {
        const int64_t r = rb + ln;
        const bool inb = r < hi;
        const uint4 rc = inb ? P.rec[r] : make_uint4(0, 0, 0, 0);
        const bool ovl = inb && (int64_t)(int32_t)rc.y > beg;
        const uint32_t ncig = rc.z & NCIG_MASK;
        // only reads with an I >= 50 op walk their CIGAR words
        const bool walk = ovl && ncig > 0 && P.spoffI[r + 1] > P.spoffI[r];
        const uint32_t *cig = walk ? P.cigar + P.off64[r] : nullptr;
        const uint64_t ib = walk ? a.ins_base[r] : 0ull;
        int cnt = 0;
        for (int pass = 0; pass < 2; pass++) {   // count, then write at the scanned offset
            int o = 0;
            if (pass == 1) {
                const uint32_t incl = wave_scan_add((uint32_t)cnt);
                o = nsel + (int)(incl - (uint32_t)cnt);
                nsel += (int)rdlane(incl, WAVE - 1);
            }
            if (walk && (pass == 0 || cnt > 0)) {
                uint32_t rp = rc.x;
                uint64_t kI = 0;
                for (uint32_t i = 0; i < ncig; i++) {
                    const uint32_t w = cig[i], op = w & 0xfu, len = w >> 4;
                    if (op == OP_INS && len >= (uint32_t)SV_MIN_LENGTH) {
                        const int64_t d = (int64_t)rp - (int64_t)R;
                        if ((d < 0 ? -d : d) <= a.pp.support_radius && (int)len <= a.pp.max_len) {
                            if (pass == 0) cnt++;
                            else if (o < a.pp.max_support) sup[o++] = (int32_t)(ib + kI);
                            else o++;
                        }
                        kI++;
                    }
                    rp += ref_adv(w);
                    if (rp > e) break;
                }
            }
        }
    }
    poa_sync();
    return nsel;
}

// Per locus (one wave each): the supporting sequences and a cost estimate, so the host can
// hand the consensus kernel its loci longest first (its per-wave time is that of the
// heaviest loci otherwise: one locus can take half the launch).
__global__ __launch_bounds__(64) void poa_support_kernel(PoaArgs a) {
    const int ln = lane_id();
    for (uint32_t li = blockIdx.x; li < a.n; li += gridDim.x) {
        const svt_locus L = a.loci[li];
        const uint32_t R = (uint32_t)uniform_i((int32_t)a.refined[li].start);
        int32_t *sup = a.supg + (uint64_t)li * (uint64_t)a.pp.max_support;
        int nsup = -1;
        uint64_t est = 0;
        if (uniform_i(L.type) == T_INS && R != SVT_NA) {
            const uint32_t pos = (uint32_t)uniform_i((int32_t)L.pos);
            const uint32_t s = pos - (uint32_t)a.prm.median, e = pos + (uint32_t)a.prm.median;   // audit.c:178
            nsup = poa_support(a, sup, uniform_i(L.chrom), s, e, R);
            const int nlist = min(nsup, a.pp.max_support);
            int cnt = 0;
            for (int q = 0; q < nlist && cnt < a.pp.max_seqs; q++) {   // one lane: nlist <= 64
                const uint32_t idx = (uint32_t)uniform_i(sup[q]);
                const uint64_t m = a.ins_off[idx + 1] - a.ins_off[idx];
                if (m >= 1) { est += m; cnt++; }
            }
        }
        if (ln == 0) {
            a.nsupg[li] = nsup;
            a.est[li] = (uint32_t)min(est, (uint64_t)0xffffffffu);
        }
    }
}

// Persistent: wave (workgroup) b owns scratch slot b and takes loci from the work queue.  A
// locus whose graph would outgrow the slot (node_cap) while still within max_nodes, or whose
// far rows exhaust the spill rows, is abandoned with status POA_DEFER; the host reruns those
// on full-size slots (node_cap = max_nodes, a spill row per node: they never defer).
constexpr int32_t POA_DEFER = 1;
constexpr uint32_t POA_PRIO_LOCI = 256;   // the heaviest loci run at raised wave priority

__global__ __launch_bounds__(64) void poa_kernel(PoaArgs a) {
    __shared__ uint8_t seq[POA_SEQ_MAX + 64];
    __shared__ PoaRing ring;
    const int ln = lane_id();
    const PoaSlot g = poa_slot(a, blockIdx.x);
    const unsigned long long tw0 = SVT_POA_DIAG ? wall_clock64() : 0ull;
    if (SVT_POA_DIAG && a.diag && ln == 0) atomicMin(a.diag + PD_T0, tw0);
    for (;;) {
        uint32_t qi = 0;
        if (ln == 0) qi = atomicAdd(a.queue, 1u);
        qi = rdlane(qi, 0);
        if (qi >= a.n) break;
        // the list runs longest first: its head bounds the launch, so it issues first on a SIMD
        if (qi < POA_PRIO_LOCI) __builtin_amdgcn_s_setprio(3);
        else __builtin_amdgcn_s_setprio(0);
        const uint32_t li = a.list ? (uint32_t)uniform_i((int32_t)a.list[qi]) : qi;
        int4 res = make_int4(-1, 0, 0, 0);
        unsigned long long t0 = SVT_POA_DIAG ? wall_clock64() : 0ull;
        const unsigned long long tl0 = t0;
        const int nsup = uniform_i(a.nsupg[li]);
        if (nsup >= 0) {
            const int32_t *sup = a.supg + (uint64_t)li * (uint64_t)a.pp.max_support;
            const int nlist = min(nsup, a.pp.max_support);
            pdiag(a.diag, PD_SUPPORT, t0);
            int n_nodes = 2, nord = 0, used = 0;
            bool defer = false;
            for (int q = 0; q < nlist && used < a.pp.max_seqs; q++) {
                const uint32_t idx = (uint32_t)uniform_i(sup[q]);
                const uint64_t o0 = a.ins_off[idx];
                const int m = uniform_i((int32_t)(a.ins_off[idx + 1] - o0));
                if (m < 1 || n_nodes - 2 + m > a.pp.max_nodes) continue;
                if (n_nodes - 2 + m > a.node_cap) { defer = true; break; }
                __syncthreads();
                for (int k = ln; k < m; k += WAVE) seq[k] = a.ins_bases[o0 + (uint64_t)k];
                __syncthreads();
                pcount(a.diag, PD_NSEQ, 1);
                if (n_nodes == 2) {
                    poa_init_chain(g, seq, m, n_nodes, nord);
                    used++;
                    pdiag(a.diag, PD_LOAD, t0);
                } else {
                    pdiag(a.diag, PD_LOAD, t0);
                    const int n = poa_align(g, ring, a.pp, seq, m, nord, a.spill_cap, a.diag);
                    if (SVT_POA_DIAG) t0 = wall_clock64();
                    if (n == -2) { defer = true; break; }   // spill rows exhausted
                    if (n >= 0) {
                        poa_fuse(g, seq, n, n_nodes, nord);
                        used++;
                    }
                    pdiag(a.diag, PD_FUSE, t0);
                }
            }
            int len = 0;
            if (defer) res = make_int4(-1, nsup, 0, POA_DEFER);
            else {
                if (used > 0) len = poa_consensus_bases(g, nord, a.out + (uint64_t)li * (uint64_t)a.cap, a.cap);
                res = make_int4(len, nsup, used, 0);
                pdiag(a.diag, PD_CONS, t0);
            }
        }
        if (ln == 0) a.res[li] = res;
        if (SVT_POA_DIAG && a.diag && ln == 0) atomicMax(a.diag + PD_LOCMAX, wall_clock64() - tl0);
        __syncthreads();
    }
    if (SVT_POA_DIAG && a.diag && ln == 0) {
        const unsigned long long tw1 = wall_clock64();
        atomicMax(a.diag + PD_T1, tw1);
        atomicMax(a.diag + PD_WAVEMAX, tw1 - tw0);
    }
}
