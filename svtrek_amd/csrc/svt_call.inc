// svt_call.inc -- discovery of DEL / INS calls from the value buckets (include/svtrek_call.h;
// included by svt_engine.hip after svt_evidence.inc, the host side is svt_call_host.inc).
//
// The items of a scan are the OP_DEL events of array S and the events of array I, both filed by
// the walk position x in 1 kb buckets per contig (svt_bucket_build.inc).  The buckets of a contig
// are contiguous in ev and in value order, so x only has to be put in order INSIDE runs of whole
// buckets; after that every (type, contig) stretch is sorted and a cluster is a run of neighbours.
// No CIGAR is walked again, no host pass touches an event, nothing is sorted globally.
//
//   segments   (call_flag_kernel + one select, ONCE per loaded pileup: the extents never change)
//              A bucket of more than CALL_H events is BIG and a segment by itself.  The other
//              buckets of a (type, contig) are cut where the CALL_H-event chunk their first event
//              lies in changes: the buckets starting in one chunk hold < 2 * CALL_H = CALL_TILE
//              events.  Every boundary is a test of a bucket and its left neighbour alone.
//   sort       (call_sort_kernel, one workgroup per segment) events -> 64-bit keys x << 28 | len;
//              non-items, types not asked for and x >= 2^30 become the all-ones sentinel.  A
//              segment of up to CALL_TILE keys is sorted in LDS, a big bucket in device memory,
//              both by the same bitonic network whose comparators all point upwards, so that the
//              slots past n never have to exist (an absent slot is a +inf that never moves).  Only
//              a contig's last bucket (every value past the others, so no bound on its range of x)
//              takes the in-memory network when it is big; any other big bucket spans 1 kb of x
//              and is ordered by a counting sort over 1024 LDS counters (call_count_sort).
//              The keys go to a scratch array at the events' own offsets, sentinels last in their
//              segment; per segment {type-contig, largest valid x + 1} goes to a table.
//   link       an exclusive max-scan of that table gives every segment the last valid x before it
//              in its (type, contig); call_head_kernel marks the cluster heads (x - prev > link, or
//              no prev); an inclusive sum of the marks numbers the clusters; call_accum_kernel
//              adds every item into its cluster's record with integer atomics (exact in any
//              order); call_pick_kernel + one select list the clusters with c >= min_support.
//   emit       (call_emit_kernel, one wave per call) the rounded means, the depth as evidence's
//              one-base region query (ev_depth), the 48-B record in 12 lanes' stores (call_store);
//              merge_lists_kernel then merges the DEL and the INS list, each in (chrom, pos) order
//              as it comes, into (chrom, pos, type) order -- a binary search per call.
// No two calls compare equal (clusters of one type and contig have disjoint x ranges, so their
// rounded means differ), and no step depends on the order of the events inside a bucket.
//   split      (len_permille > 0 only: the kernels at the end of this file, between accum and pick)
//              the clusters that can hold a cut by length are sorted by len and cut into groups, one
//              call per group of >= min_support items, in (chrom, pos, type, len) order.
constexpr uint32_t CALL_H = 1024, CALL_TILE = 2 * CALL_H;
constexpr int CALL_T = 256;                       // threads of the per-segment kernels
constexpr uint64_t CALL_NONE = ~0ull;             // the sentinel key
static_assert(sizeof(svt_call) == 48, "svt_call is copied as three 16-B words");

struct CallAcc {   // 40 B, zeroed before every scan (the two minima are kept as maxima of ~v)
    unsigned long long sx, slen;
    uint32_t cnt, nlen_lo, len_hi, nx_lo, x_hi, seg;
};

struct CallArgs {
    BkIndex bk;
    DevPileup pile;
    int32_t nt;
    uint32_t n_s;                 // S events (the I events' keys follow them in the scratch)
    uint64_t n_seg;
    const uint64_t *seg;          // [n_seg] first combined bucket (array * nbk + bucket) of every segment
    unsigned long long *keys;     // [n_s + n_i]
    uint32_t *cid;                // [n_s + n_i] head marks, then cluster numbers (1-based, inclusive)
    unsigned long long *tmax;     // [n_seg] (type * nt + contig) << 32 | largest valid x + 1 (0: none)
    const unsigned long long *tprev;   // [n_seg] its exclusive max-scan
    CallAcc *acc;
    uint32_t *pick;               // the called clusters in cluster order, *pick_n of them
    uint32_t *pick_n;
    unsigned long long *stats;    // events, skipped, big buckets
    uint32_t link, min_support, types;
    uint32_t permille;            // svt_call_params.len_permille
    uint32_t *first;              // [clusters] every cluster's first key slot; NULL unless the scan splits by length
};

// The contig of bucket g (cbase is ascending, cbase[0] == 0).
__device__ __forceinline__ int call_contig(const BkIndex &B, int nt, uint64_t g) {
    int lo = 0, hi = nt;
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (B.cbase[m] <= g) lo = m;
        else hi = m;
    }
    return lo;
}

__global__ __launch_bounds__(256) void call_flag_kernel(BkIndex B, int nt, uint8_t *flag) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= 2 * B.nbk) return;
    const uint64_t g = j >= B.nbk ? j - B.nbk : j;
    const uint32_t *off = B.off + (uint64_t)(j >= B.nbk ? BA_I : BA_S) * (B.nbk + 1);
    const uint32_t o0 = off[g], n = off[g + 1] - o0;
    bool f = B.cbase[call_contig(B, nt, g)] == g || n > CALL_H;
    if (!f) {
        const uint32_t q0 = off[g - 1];
        f = o0 - q0 > CALL_H || (o0 - off[0]) / CALL_H != (q0 - off[0]) / CALL_H;
    }
    flag[j] = f ? 1 : 0;
}

// One segment: its array, events [E0, E1), first key slot p0 and type-contig number sg.
struct CallSeg {
    uint32_t E0, n, p0, sg;
    int a2;
    bool last;   // the segment starts at its contig's last bucket (every value past the others)
};
__device__ __forceinline__ CallSeg call_seg(const CallArgs &a, uint64_t k) {
    const uint64_t j0 = a.seg[k], j1 = k + 1 < a.n_seg ? a.seg[k + 1] : 2 * a.bk.nbk;
    CallSeg s;
    s.a2 = j0 >= a.bk.nbk ? 1 : 0;
    const uint64_t g0 = j0 - (s.a2 ? a.bk.nbk : 0), g1 = g0 + (j1 - j0);
    const uint32_t *off = a.bk.off + (uint64_t)(s.a2 ? BA_I : BA_S) * (a.bk.nbk + 1);
    s.E0 = off[g0];
    s.n = off[g1] - s.E0;
    s.p0 = s.E0 - off[0] + (s.a2 ? a.n_s : 0u);
    const int t = call_contig(a.bk, a.nt, g0);
    s.sg = (uint32_t)s.a2 * (uint32_t)a.nt + (uint32_t)t;
    s.last = g0 + 1 == a.bk.cbase[t] + a.bk.cnb[t];
    return s;
}

// The bitonic network with every comparator pointing upwards, on n <= P = 2^k slots: a comparator
// whose upper slot is >= n is skipped (the absent slots are +inf and never move).
__device__ __forceinline__ void call_cmpswap(unsigned long long *k, uint32_t lo, uint32_t hi, uint32_t n) {
    if (hi < n) {
        const unsigned long long x = k[lo], y = k[hi];
        if (x > y) { k[lo] = y; k[hi] = x; }
    }
}
__device__ __forceinline__ void call_bitonic(unsigned long long *k, uint32_t n) {
    uint32_t P = 1;
    while (P < n) P <<= 1;
    for (uint32_t w = 2; w <= P; w <<= 1) {
        const uint32_t h = w >> 1;
        for (uint32_t i = threadIdx.x; i < P / 2; i += CALL_T) {      // the mirror step
            const uint32_t b = i / h, r = i % h;
            call_cmpswap(k, b * w + r, b * w + w - 1 - r, n);
        }
        __syncthreads();
        for (uint32_t d = w >> 2; d >= 1; d >>= 1) {
            for (uint32_t i = threadIdx.x; i < P / 2; i += CALL_T) {
                const uint32_t lo = (i / d) * 2 * d + i % d;
                call_cmpswap(k, lo, lo + d, n);
            }
            __syncthreads();
        }
    }
}

// Keys of segment s into k (LDS, or the scratch itself for a big bucket), sorted; the sorted keys'
// valid count into cnt[2], the items and the skipped ones into cnt[0] and cnt[1].
template <bool BIG>
__device__ __forceinline__ void call_sort_body(const CallArgs &a, const CallSeg &s, unsigned long long *k, uint32_t *cnt) {
    const uint32_t want = s.a2 ? OP_INS : OP_DEL;
    const bool asked = (a.types >> (s.a2 ? SVT_INS : SVT_DEL)) & 1u;
    uint32_t items = 0, skipped = 0, valid = 0;
    for (uint32_t i = threadIdx.x; i < s.n; i += CALL_T) {
        const uint4 v = a.bk.ev[s.E0 + i];
        const bool item = asked && (v.y & 0xfu) == want;
        const bool sat = v.x >= IX_SAT;
        items += item ? 1u : 0u;
        skipped += item && sat ? 1u : 0u;
        valid += item && !sat ? 1u : 0u;
        k[i] = item && !sat ? ((unsigned long long)v.x << 28) | (v.y >> 4) : CALL_NONE;
    }
    if (items) atomicAdd(&cnt[0], items);
    if (skipped) atomicAdd(&cnt[1], skipped);
    if (valid) atomicAdd(&cnt[2], valid);
    __syncthreads();
    call_bitonic(k, s.n);
    if (!BIG)
        for (uint32_t i = threadIdx.x; i < s.n; i += CALL_T) a.keys[s.p0 + i] = k[i];
}

// One event of segment s as a key: the sentinel for non-items, types not asked for and x >= 2^30.
__device__ __forceinline__ unsigned long long call_key(const CallArgs &a, const CallSeg &s, const uint4 &v) {
    const bool asked = (a.types >> (s.a2 ? SVT_INS : SVT_DEL)) & 1u;
    const bool ok = asked && (v.y & 0xfu) == (s.a2 ? OP_INS : OP_DEL) && v.x < IX_SAT;
    return ok ? ((unsigned long long)v.x << 28) | (v.y >> 4) : CALL_NONE;
}

// A big bucket that is not its contig's last: every x lies in the bucket's own 1 kb, so a counting
// sort by the x offset orders it in two passes over the events whatever their number -- a histogram
// of 1024 LDS counters, their exclusive scan (wave 0, 16 slots a lane), then every key to the next
// free slot of its x.  Keys of one x land in any order: nothing downstream reads it (the cluster
// records are sums, minima and maxima).  The sentinels go behind the valid keys.
__device__ __forceinline__ void call_count_sort(const CallArgs &a, const CallSeg &s, uint32_t *hist, uint32_t *cnt) {
    const uint32_t want = s.a2 ? OP_INS : OP_DEL;
    const bool asked = (a.types >> (s.a2 ? SVT_INS : SVT_DEL)) & 1u;
    for (uint32_t i = threadIdx.x; i < CALL_H; i += CALL_T) hist[i] = 0;
    __syncthreads();
    uint32_t items = 0, skipped = 0, valid = 0;
    for (uint32_t i = threadIdx.x; i < s.n; i += CALL_T) {
        const uint4 v = a.bk.ev[s.E0 + i];
        const bool item = asked && (v.y & 0xfu) == want;
        const bool sat = v.x >= IX_SAT;
        items += item ? 1u : 0u;
        skipped += item && sat ? 1u : 0u;
        valid += item && !sat ? 1u : 0u;
        if (item && !sat) atomicAdd(&hist[v.x & (CALL_H - 1u)], 1u);
    }
    if (items) atomicAdd(&cnt[0], items);
    if (skipped) atomicAdd(&cnt[1], skipped);
    if (valid) atomicAdd(&cnt[2], valid);
    __syncthreads();
    if (threadIdx.x < WAVE) {   // counts -> first slots
        constexpr uint32_t PER = CALL_H / WAVE;
        uint32_t sum = 0;
        for (uint32_t j = 0; j < PER; j++) sum += hist[threadIdx.x * PER + j];
        uint32_t at = wave_scan_add(sum) - sum;
        for (uint32_t j = 0; j < PER; j++) {
            const uint32_t c = hist[threadIdx.x * PER + j];
            hist[threadIdx.x * PER + j] = at;
            at += c;
        }
    }
    __syncthreads();
    const uint32_t nv = cnt[2];
    for (uint32_t i = threadIdx.x; i < s.n; i += CALL_T) {
        const unsigned long long key = call_key(a, s, a.bk.ev[s.E0 + i]);
        const uint32_t at = key != CALL_NONE ? atomicAdd(&hist[(uint32_t)(key >> 28) & (CALL_H - 1u)], 1u)
                                             : nv + atomicAdd(&cnt[3], 1u);
        if (at < s.n) a.keys[s.p0 + at] = key;   // (always: the two passes read the same events)
    }
    __syncthreads();
}

__global__ __launch_bounds__(CALL_T) void call_sort_kernel(CallArgs a) {
    __shared__ unsigned long long lk[CALL_TILE];
    __shared__ uint32_t hist[CALL_H];
    __shared__ uint32_t cnt[4];   // items, skipped, valid keys, sentinels placed (call_count_sort)
    const CallSeg s = call_seg(a, blockIdx.x);
    if (s.n == 0) {
        if (threadIdx.x == 0) a.tmax[blockIdx.x] = (unsigned long long)s.sg << 32;
        return;
    }
    if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
    __syncthreads();
    const bool big = s.n > CALL_TILE;   // (more than CALL_H events in a segment: it is one bucket)
    if (big && !s.last) call_count_sort(a, s, hist, cnt);
    else if (big) call_sort_body<true>(a, s, a.keys + s.p0, cnt);
    else call_sort_body<false>(a, s, lk, cnt);
    if (threadIdx.x == 0) {   // (after the sort's last barrier, or -- n == 1 -- this thread's own store)
        const uint32_t nv = cnt[2];
        const uint32_t top = nv ? (uint32_t)((big ? a.keys[s.p0 + nv - 1] : lk[nv - 1]) >> 28) + 1u : 0u;
        a.tmax[blockIdx.x] = (unsigned long long)s.sg << 32 | top;
        if (cnt[0]) atomicAdd(&a.stats[0], (unsigned long long)cnt[0]);
        if (cnt[1]) atomicAdd(&a.stats[1], (unsigned long long)cnt[1]);
        if (big) atomicAdd(&a.stats[2], 1ull);
    }
}

__global__ __launch_bounds__(CALL_T) void call_head_kernel(CallArgs a) {
    const CallSeg s = call_seg(a, blockIdx.x);
    const unsigned long long tp = a.tprev[blockIdx.x];
    const bool have = (uint32_t)(tp >> 32) == s.sg && (uint32_t)tp != 0u;
    for (uint32_t i = threadIdx.x; i < s.n; i += CALL_T) {
        const unsigned long long key = a.keys[s.p0 + i];
        bool head = false;
        if (key != CALL_NONE) {
            const uint32_t x = (uint32_t)(key >> 28);
            if (i > 0) head = x - (uint32_t)(a.keys[s.p0 + i - 1] >> 28) > a.link;   // (valid: the sentinels come last)
            else head = !have || x - ((uint32_t)tp - 1u) > a.link;
        }
        a.cid[s.p0 + i] = head ? 1u : 0u;
    }
}

__global__ __launch_bounds__(CALL_T) void call_accum_kernel(CallArgs a) {
    const CallSeg s = call_seg(a, blockIdx.x);
    for (uint32_t i = threadIdx.x; i < s.n; i += CALL_T) {
        const uint32_t p = s.p0 + i;
        const unsigned long long key = a.keys[p];
        const uint32_t c = a.cid[p];
        if (key == CALL_NONE || c == 0u) continue;   // (c >= 1: a valid key is a head or follows one)
        const uint32_t x = (uint32_t)(key >> 28), len = (uint32_t)key & 0xfffffffu;
        CallAcc *q = a.acc + (c - 1u);
        if (c != (p ? a.cid[p - 1] : 0u)) {
            q->seg = s.sg;
            if (a.first) a.first[c - 1u] = p;
        }
        atomicAdd(&q->cnt, 1u);
        atomicAdd(&q->sx, (unsigned long long)x);
        atomicAdd(&q->slen, (unsigned long long)len);
        atomicMax(&q->nlen_lo, ~len);
        atomicMax(&q->len_hi, len);
        atomicMax(&q->nx_lo, ~x);
        atomicMax(&q->x_hi, x);
    }
}

// flag[c]: cluster c is a call; *n_del: the calls among the first n_s_clusters clusters (array S's: the
// DEL calls), one atomic per wave.
__global__ __launch_bounds__(256) void call_pick_kernel(CallArgs a, uint32_t n_clusters, uint32_t n_s_clusters, uint8_t *flag,
                                                        uint32_t *n_del) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    const bool call = c < n_clusters && a.acc[c].cnt >= a.min_support;
    if (c < n_clusters) flag[c] = call ? 1 : 0;
    const uint64_t m = ballot(call && c < n_s_clusters);
    if (m && lane_id() == 0) atomicAdd(n_del, (uint32_t)__popcll(m));
}

// A call record's twelve words, one store each from the wave's first twelve lanes.
__device__ __forceinline__ void call_store(svt_call *dst, const uint32_t (&w)[12]) {
    const int ln = lane_id();
    uint32_t word = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) word = ln == i ? w[i] : word;
    if (ln < 12) reinterpret_cast<uint32_t *>(dst)[ln] = word;
}
// One thread copies a record: three 16-B words.
__device__ __forceinline__ void call_copy(svt_call *dst, const svt_call *src) {
    const uint4 *s = reinterpret_cast<const uint4 *>(src);
    uint4 *d = reinterpret_cast<uint4 *>(dst);
    d[0] = s[0], d[1] = s[1], d[2] = s[2];
}

// One wave per call.  REARR: the rearrangement index's rows S / I are DUP / INV, both ending at mean(x + len).
template <bool REARR>
__global__ __launch_bounds__(64 * WPB) void call_emit_kernel(CallArgs a, uint32_t n_calls, svt_call *out) {
    const uint32_t g = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (g >= n_calls) return;
    const CallAcc q = a.acc[(uint32_t)uniform_i((int32_t)a.pick[g])];
    const unsigned long long c = q.cnt, h = c / 2;
    const int ri = q.seg >= (uint32_t)a.nt ? 1 : 0, tid = (int)(q.seg - (ri ? (uint32_t)a.nt : 0u));   // (ri: a cluster of row I)
    const uint32_t pos = (uint32_t)uniform_i((int32_t)(uint32_t)((q.sx + h) / c));
    const uint32_t len = (uint32_t)((q.slen + h) / c);
    const uint32_t end = REARR ? (uint32_t)((q.sx + q.slen + h) / c) : ri ? pos + 1u : (uint32_t)((q.sx + q.slen + c + h) / c);
    const uint32_t depth = ev_depth(a.pile, tid, pos);
    const uint32_t w[12] = {(uint32_t)(REARR ? (ri ? SVT_INV : SVT_DUP) : (ri ? SVT_INS : SVT_DEL)), (uint32_t)(tid + 1), pos, end, q.cnt,
                            depth, len, ~q.nlen_lo, q.len_hi, ~q.nx_lo, q.x_hi, 0u};
    call_store(out + g, w);
}

// Two sorted lists into one: la[0 .. na) and lb[0 .. nb), each in (chrom, pos, type code[, len]) order, every
// type code of la below every one of lb, so (chrom, pos) alone decides: a call of la goes behind the calls of lb
// strictly before it, a call of lb behind those of la at or before it.  One thread per call.  (la, lb) = a pass's
// (INS, DEL) calls, the (DEL / INS, INV / DUP) lists of a scan with rearr != 0, (the others, the BND calls).
__global__ __launch_bounds__(256) void merge_lists_kernel(const svt_call *la, uint32_t na, const svt_call *lb, uint32_t nb, svt_call *out) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= na + nb) return;
    const bool first = g < na;
    const svt_call *mine = first ? la + g : lb + (g - na), *other = first ? lb : la;
    auto key = [](const svt_call &c) { return (unsigned long long)(uint32_t)c.chrom << 32 | c.pos; };
    const unsigned long long k = key(*mine);
    uint32_t lo = 0, hi = first ? nb : na;
    while (lo < hi) {
        const uint32_t m = lo + (hi - lo) / 2;
        const unsigned long long o = key(other[m]);
        if (first ? o < k : o <= k) lo = m + 1;
        else hi = m;
    }
    call_copy(out + (first ? g : g - na) + lo, mine);
}

// ---- splitting the start clusters by length (svt_call_params.len_permille = P > 0) ----------------
// Between call_accum_kernel and call_pick_kernel.  A cluster whose own len range cannot hold a cut,
// or with fewer than min_support items, stays as it is; the others are the CANDIDATES:
//   cand       (call_cand_kernel + one select + one sum) the candidates from their CallAcc records,
//              their item counts summed into the offsets of a scratch for their sorted keys.
//   split      (call_split_kernel, one workgroup per candidate) the candidate's items are the valid
//              keys of its cluster number from its first slot on (the sentinels of the segments it
//              runs over are skipped), gathered as len << 30 | x and sorted by call_bitonic -- in LDS
//              up to CALL_TILE keys, else in the scratch itself.  A key whose len is more than
//              max(link, lo * P / 1000) past its left neighbour's heads a GROUP; the groups are counted.
//   units      every cluster is 1 unit, a candidate as many as it has groups; an inclusive sum over
//              the clusters numbers the units in cluster order.
//   group      (call_group_kernel, one workgroup per candidate) a segmented reduction over the sorted
//              keys: a thread keeps the sums of the group it is in and adds them to the group's
//              record when its next key belongs to another group -- a candidate of two alleles costs
//              a few atomics a thread, whatever its size.
//   order      (call_order_kernel, one workgroup per candidate) the groups come in len order; their
//              keys pos << 32 | group go through the same network and the records to the candidate's
//              units in (pos, len) order.  call_unit_kernel copies the other clusters' records.
// call_pick_kernel, call_emit_kernel and merge_lists_kernel then run on the units as they do on the
// clusters: units of different clusters keep the clusters' order, so both lists are in (chrom, pos,
// len) order and the merge gives (chrom, pos, type, len).  Groups of one cluster have disjoint len
// ranges more than link apart, so their rounded mean len differ: no two calls compare equal.
struct CallSplit {
    const uint8_t *cflag;         // [clusters] 1: a candidate
    const uint32_t *cand;         // the candidates in cluster order (one workgroup each)
    const uint32_t *kend;         // [clusters] inclusive sum of the candidates' item counts: where a candidate's sorted keys end
    unsigned long long *skeys;    // the candidates' keys len << 30 | x, sorted; then call_order_kernel's scratch
    uint32_t *unit;               // [clusters] units of every cluster, then their inclusive sum
    CallAcc *gacc;                // [units] a candidate's groups in len order at its units (zeroed)
    CallAcc *uacc;                // [units] every unit's record, a candidate's in (pos, len) order
    unsigned long long *stats;    // split, groups, big
    uint32_t n_keys;              // key slots (n_s + n_i)
};

// Is there a cut between the sorted neighbours lo <= hi?  (lo < 2^28 and P <= 1000: the quotient fits.)
__device__ __forceinline__ bool call_len_cut(uint32_t lo, uint32_t hi, uint32_t link, uint32_t permille) {
    const uint32_t rel = (uint32_t)((unsigned long long)lo * permille / 1000u);
    return hi - lo > max(link, rel);
}

__global__ __launch_bounds__(256) void call_cand_kernel(CallArgs a, uint32_t n_clusters, uint8_t *cflag, uint32_t *kcnt,
                                                        uint32_t *unit) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= n_clusters) return;
    const CallAcc *q = a.acc + c;
    const uint32_t cnt = q->cnt;
    const bool cand = cnt >= a.min_support && call_len_cut(~q->nlen_lo, q->len_hi, a.link, a.permille);
    cflag[c] = cand ? 1 : 0;
    kcnt[c] = cand ? cnt : 0u;
    unit[c] = 1u;
}

__global__ __launch_bounds__(CALL_T) void call_split_kernel(CallArgs a, CallSplit sp) {
    __shared__ unsigned long long lk[CALL_TILE];
    __shared__ uint32_t got, ng;
    const uint32_t c = sp.cand[blockIdx.x], cnt = a.acc[c].cnt, off = sp.kend[c] - cnt;
    const bool big = cnt > CALL_TILE;
    unsigned long long *k = big ? sp.skeys + off : lk;
    if (threadIdx.x == 0) got = 0, ng = 0;
    __syncthreads();
    const int ln = lane_id();
    for (uint32_t base = a.first[c]; base < sp.n_keys; base += CALL_T) {   // (ends at cnt keys: the cluster has them)
        const uint32_t p = base + threadIdx.x;
        unsigned long long key = CALL_NONE;
        if (p < sp.n_keys && a.cid[p] == c + 1u) key = a.keys[p];
        const uint64_t m = ballot(key != CALL_NONE);
        uint32_t at = 0;
        if (m && ln == 0) at = atomicAdd(&got, (uint32_t)__popcll(m));
        at = rdlane(at, 0) + (uint32_t)__popcll(m & ((1ull << ln) - 1ull));
        if (key != CALL_NONE && at < cnt) k[at] = (key & 0xfffffffull) << 30 | key >> 28;
        __syncthreads();
        const uint32_t have = got;
        __syncthreads();
        if (have >= cnt) break;
    }
    call_bitonic(k, cnt);
    uint32_t heads = 0;
    for (uint32_t i = threadIdx.x; i < cnt; i += CALL_T) {
        const unsigned long long key = k[i];
        heads += i == 0 || call_len_cut((uint32_t)(k[i - 1] >> 30), (uint32_t)(key >> 30), a.link, a.permille) ? 1u : 0u;
        if (!big) sp.skeys[off + i] = key;
    }
    if (heads) atomicAdd(&ng, heads);
    __syncthreads();
    if (threadIdx.x == 0) {
        sp.unit[c] = ng;
        if (ng > 1) atomicAdd(&sp.stats[0], 1ull);
        atomicAdd(&sp.stats[1], (unsigned long long)ng);
        if (big) atomicAdd(&sp.stats[2], 1ull);
    }
}

__global__ __launch_bounds__(CALL_T) void call_group_kernel(CallArgs a, CallSplit sp) {
    __shared__ uint32_t wsum[CALL_T / WAVE];
    const uint32_t c = sp.cand[blockIdx.x], cnt = a.acc[c].cnt, seg = a.acc[c].seg;
    const unsigned long long *k = sp.skeys + (sp.kend[c] - cnt);
    CallAcc *g = sp.gacc + (c ? sp.unit[c - 1] : 0u);
    const int ln = lane_id(), w = threadIdx.x / WAVE;
    uint32_t carry = 0;                                   // groups before this round's keys
    uint32_t mine = 0, n = 0, len_lo = 0, len_hi = 0, x_lo = 0, x_hi = 0;   // the group this thread is in, its sums so far
    unsigned long long sx = 0, slen = 0;
    auto flush = [&]() {
        if (n == 0) return;
        CallAcc *q = g + mine;
        atomicAdd(&q->cnt, n);
        atomicAdd(&q->sx, sx);
        atomicAdd(&q->slen, slen);
        atomicMax(&q->nlen_lo, ~len_lo);
        atomicMax(&q->len_hi, len_hi);
        atomicMax(&q->nx_lo, ~x_lo);
        atomicMax(&q->x_hi, x_hi);
        n = 0, sx = 0, slen = 0;
    };
    for (uint32_t base = 0; base < cnt; base += CALL_T) {
        const uint32_t i = base + threadIdx.x;
        const bool in = i < cnt;
        const unsigned long long key = in ? k[i] : 0ull;
        const uint32_t len = (uint32_t)(key >> 30), x = (uint32_t)key & 0x3fffffffu;
        const bool head = in && (i == 0 || call_len_cut((uint32_t)(k[i - 1] >> 30), len, a.link, a.permille));
        const uint64_t m = ballot(head);
        if (ln == 0) wsum[w] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = carry;
        for (int v = 0; v < CALL_T / WAVE; v++) {
            const uint32_t t = wsum[v];
            carry += t;
            before += v < w ? t : 0u;
        }
        __syncthreads();
        if (!in) continue;   // (every round but the last is full, and the last ends the loop)
        const uint32_t gi = before + (uint32_t)__popcll(m & ((2ull << ln) - 1ull)) - 1u;   // (key 0 is a head)
        if (n == 0 || gi != mine) {
            flush();
            mine = gi, len_lo = len, x_lo = x_hi = x;
        }
        n++, sx += x, slen += len;
        len_hi = len;                                     // (the keys ascend by len)
        x_lo = min(x_lo, x), x_hi = max(x_hi, x);
        if (head) g[gi].seg = seg;
    }
    flush();
}

__global__ __launch_bounds__(256) void call_unit_kernel(CallArgs a, CallSplit sp, uint32_t n_clusters) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= n_clusters || sp.cflag[c]) return;
    sp.uacc[c ? sp.unit[c - 1] : 0u] = a.acc[c];
}

__global__ __launch_bounds__(CALL_T) void call_order_kernel(CallArgs a, CallSplit sp) {
    __shared__ unsigned long long lk[CALL_TILE];
    const uint32_t c = sp.cand[blockIdx.x], ub = c ? sp.unit[c - 1] : 0u, ng = sp.unit[c] - ub;
    const CallAcc *g = sp.gacc + ub;
    CallAcc *u = sp.uacc + ub;
    if (ng == 1) {
        if (threadIdx.x == 0) u[0] = g[0];
        return;
    }
    unsigned long long *k = ng > CALL_TILE ? sp.skeys + (sp.kend[c] - a.acc[c].cnt) : lk;   // (ng <= cnt keys: the sorted keys are spent)
    for (uint32_t i = threadIdx.x; i < ng; i += CALL_T) {
        const unsigned long long n = g[i].cnt;
        k[i] = (g[i].sx + n / 2) / n << 32 | i;
    }
    __syncthreads();
    call_bitonic(k, ng);
    for (uint32_t i = threadIdx.x; i < ng; i += CALL_T) u[i] = g[(uint32_t)k[i]];
}
