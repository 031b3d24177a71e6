// svt_devmem.inc -- host only: the owners of what the engine's host code allocates on the device
// (included by svt_engine.hip after the device code and before svt_ctx), and the host-side records
// of the side modes' scratch.  Nothing here is a kernel argument: KArgs, IxArgs, BkBuild, CallArgs,
// PoaArgs and BdCols keep raw pointers, filled from these owners at launch.

// One hipMalloc allocation and its capacity in elements.  Move-only; freed by reset() and the
// destructor, on whatever device is current then (every entry point runs under its DevGuard).
// Allocation returns the hipError_t; the caller turns it into its own status and message.
template <typename T>
class DevBuf {
    T *p_ = nullptr;
    size_t cap_ = 0;

public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_, cap_ = o.cap_;
            o.p_ = nullptr, o.cap_ = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() {
        if (p_) (void)hipFree((void *)p_);
        p_ = nullptr, cap_ = 0;
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t cap() const { return cap_; }
    // At least n elements, contents not kept: nothing when n <= cap(), else the old block is freed
    // first and exactly n allocated (the buffer is empty when that fails).
    hipError_t reserve(size_t n) {
        if (n <= cap_) return hipSuccess;
        reset();
        const hipError_t e = hipMalloc((void **)&p_, n * sizeof(T));
        if (e != hipSuccess) p_ = nullptr;
        else cap_ = n;
        return e;
    }
    // At least `need` elements, the first `keep` kept (the BAM decoder's buffers): a new block of
    // max(need, 1.5 x cap()) and a device copy.  The buffer is unchanged when either fails.
    hipError_t grow(size_t need, size_t keep = 0) {
        if (need <= cap_) return hipSuccess;
        DevBuf q;
        hipError_t e = q.reserve(std::max(need, cap_ + cap_ / 2));
        if (e == hipSuccess && keep && p_) e = hipMemcpy(q.p_, p_, keep * sizeof(T), hipMemcpyDeviceToDevice);
        if (e == hipSuccess) *this = std::move(q);
        return e;
    }
};

// One HIP event, created on demand.
struct DevEvent {
    hipEvent_t e = nullptr;
    DevEvent() = default;
    DevEvent(const DevEvent &) = delete;
    DevEvent &operator=(const DevEvent &) = delete;
    ~DevEvent() {
        if (e) (void)hipEventDestroy(e);
    }
    hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
};

// What a loaded pileup keeps on the device, by owner (svt_load_host.inc fills all three).  Each owner
// has one function that gives the kernels' read-only view of it; the builds' argument structs
// (ix_args, bk_args) take the same view and, for what they write, the owner's buffers.

// The read columns, as uploaded from the host pass (svt_loadprep.h); nothing rebuilds them.
struct ReadCols {
    DevBuf<int32_t> d_pos, d_emax;
    DevBuf<uint4> d_rec;
    DevBuf<uint8_t> d_clip8;          // per read its clip bits (rec.z >> 30) alone: the census's 1 B instead of 16
    DevBuf<uint64_t> d_off64;         // stream offsets [n_reads + 1]
    DevBuf<int64_t> d_tid_off, d_bkt_off;
    DevBuf<uint2> d_bkt;
    DevBuf<uint32_t> d_cigar;         // CIGAR stream
    void view(DevPileup &v) const {
        v.pos = d_pos, v.emax = d_emax, v.rec = d_rec, v.off64 = d_off64;
        v.tid_off = d_tid_off, v.bkt_off = d_bkt_off, v.bkt = d_bkt, v.cigar = d_cigar;
    }
};

// The span-list index (svt_index.inc, svt_index2.inc): the lists, and the ranges, totals and scratch
// of their build.
struct SpanIndex {
    DevBuf<uint64_t> d_part;          // [n_ranges + 1]
    uint32_t n_ranges = 0;
    DevBuf<IxTot> d_agg;              // range (group) totals
    DevBuf<IxTot> d_bsum, d_bpre;     // their sums per block of IX_BLK, the blocks' exclusive scan
    size_t n_bsum = 0;
    bool bsum_dirty = false;          // a build stopped between its walk (which adds into d_bsum) and the
                                      // scan (which zeroes it again): the next build clears it first
    DevBuf<uint4> d_scr;              // stream walk: staged events / offsets per range, overflow flags
    DevBuf<uint2> d_scrh;
    DevBuf<uint32_t> d_ovf;
    DevBuf<uint2> d_cnt;              // [n_reads] lane-per-read census -> emit (svt_index2.inc)
    uint32_t n_groups = 0;            // 64-read groups of the lane-per-read index
    DevBuf<uint64_t> d_tot;
    uint64_t n_evD = 0, n_evI = 0;
    DevBuf<uint64_t> d_spoffD, d_spoffI;   // span walk
    DevBuf<uint4> d_spD, d_spI;
    void view(DevPileup &v) const { v.spoffD = d_spoffD, v.spoffI = d_spoffI, v.spD = d_spD, v.spI = d_spI; }
};

// The value-bucketed event index (svt_bucket.inc, svt_bucket_build.inc).
struct ValueBuckets {
    bool ready = false;               // built for the loaded pileup
    uint64_t n = 0;                   // buckets per array (every contig's)
    DevBuf<uint32_t> d_off;           // [BA_N][n + 1] extents (indices into d_ev)
    DevBuf<uint32_t> d_cur;           // [BA_N][n + 1] cursors of direct builds (k * count before build k)
    DevBuf<uint32_t> d_cap;           // [BA_N][n + 1] cursors of captured builds (zeroed by the graph)
    DevBuf<int32_t> d_pm;             // [3][n + 1] prefix max of the BELOW keys
    DevBuf<uint4> d_ev;               // every array's events
    uint64_t events[BA_N] = {};
    DevBuf<uint64_t> d_base;          // [n_targets] first bucket of contig t
    DevBuf<uint32_t> d_nb;            // [n_targets] its buckets
    DevBuf<uint32_t> d_maxd;          // [n_targets] its longest D > 50 op
    uint32_t builds = 0;              // filing passes so far (the cursors' epoch)
    uint32_t nev = 0;                 // d_ev's events (every array's)
    BkIndex view() const { return BkIndex{d_ev, d_off, d_pm, d_base, d_nb, d_maxd, n, ready ? 1 : 0}; }
};

// The segments of one index a scan runs on (call_prepare, svt_call_host.inc): they depend on the extents.
struct CallSegs {
    bool ready = false;
    uint64_t n_seg = 0;
    DevBuf<uint64_t> d_seg;
};

// One index in the value buckets' shape, derived from the loaded pileup for svt_call_scan to run on
// (svt_callindex.inc; callindex_build, svt_callindex_host.inc, is the only code that fills one).
struct CallIndex {
    bool built = false;
    DevBuf<uint4> d_ev;               // array S's events, then array I's
    DevBuf<uint32_t> d_off;           // [BA_N][bk_n + 1], rows S and I filled
    uint64_t events[2] = {};          // S / I events
    CallSegs segs;                    // its own segments
    // Not built, nothing allocated.  The caller synchronises first where a launch may still read it.
    void drop() { *this = CallIndex{}; }
};

// svt_call_scan's scratch (svt_call.inc, svt_call_host.inc): nothing allocated before the first scan
// of a loaded pileup, gone with the pileup.
struct CallScratch {
    bool scanned = false;          // svt_call_scan ran on this pileup (svt_genotype_calls)
    CallSegs segs;                 // the plain buckets'
    DevBuf<unsigned long long> d_keys, d_tmax, d_tprev;
    DevBuf<uint32_t> d_cid, d_pick;
    DevBuf<uint32_t> d_ctr;        // a pass's counters, CALL_NCTR words zeroed when it begins: the device side of CallCtr
    DevBuf<CallAcc> d_acc;
    DevBuf<uint8_t> d_tmp;         // hipcub's temporary storage
    DevBuf<uint8_t> d_flag;        // per cluster: a call
    DevBuf<svt_call> d_calls, d_raw;   // the scan's calls in order / a pass's as emitted
    // (a scan's stages -- the view's pass, the rearrangement pass, the BND stage -- each hand a sorted list on)
    DevBuf<svt_call> d_list1, d_list2; // the list after the first / second stage where another follows; the last one's is d_calls
    uint64_t n_calls = 0;
    // the split by length (len_permille > 0): nothing allocated before the first such scan
    DevBuf<uint32_t> d_first, d_cand, d_kend, d_unit;   // per cluster: first key slot / candidates / their keys' ends / units
    DevBuf<uint8_t> d_cflag;       // per cluster: a candidate
    DevBuf<unsigned long long> d_skeys;   // the candidates' sorted keys
    DevBuf<CallAcc> d_gacc, d_uacc;       // per unit: the groups as accumulated / every unit in order
    // The derived indexes: nothing allocated before the first scan that asks for one, untouched by
    // svt_reindex; `stats` are the build's.
    // the merged index (merge_gap > 0; svt_callmerge.inc, svt_callmerge_host.inc): rebuilt when (gap, min) change
    struct Merged : CallIndex {
        uint32_t gap = 0, min_len = 0;    // what it was built for
        svt_call_merge_stats stats{};
    } mg;
    // the segment table (svt_load_junctions) and the union index (junctions = 1; svt_junction.inc,
    // svt_junction_host.inc): rebuilt when the table or the base view's (merge_gap, merge_min) change
    struct Junction : CallIndex {
        bool loaded = false;              // a table for the loaded pileup (n == 0 included)
        uint64_t n = 0, rows = 0;         // its records and segment rows
        DevBuf<uint64_t> d_toff;          // [n + 1]
        DevBuf<svt_junction_seg> d_tseg;  // [rows]
        uint32_t gap = 0, min_len = 0;    // the base view it was built on (gap 0: the plain buckets)
        svt_call_junction_stats stats{};
    } jn;
    // the rearrangement index (rearr != 0; svt_rearr.inc, svt_rearr_host.inc): rebuilt when the table changes
    struct Rearr : CallIndex {
        DevBuf<svt_call> d_calls;         // the second pass's INV / DUP calls before their merge with the first stage's list
        svt_call_rearr_stats stats{};
    } rr;
    // the BND item list (bnd = 1; svt_bnd.inc, svt_bnd_host.inc): no buckets, one list in (class, x) order;
    // rebuilt when the table changes.  The scratch of its scans lives and dies with it.
    struct Bnd {
        bool built = false;
        uint64_t n_items = 0;             // kept items
        DevBuf<unsigned long long> d_cls, d_xy;   // [n_items] tid_lo << 33 | tid_hi << 2 | o;  x << 32 | y
        svt_call_bnd_stats stats{};       // of the build: items, skipped, classes, build_ms
        // per scan
        DevBuf<uint32_t> d_cid, d_gid;    // [n_items] head marks, then start cluster / group numbers (1-based)
        DevBuf<unsigned long long> d_key, d_key2, d_ccls;   // cluster << 30 | y, as built / by y; [clusters] class words
        DevBuf<uint32_t> d_x, d_x2;       // x beside the keys
        DevBuf<BndAcc> d_acc;             // [groups]
        DevBuf<uint8_t> d_flag;           // per group: a call
        DevBuf<uint32_t> d_pick, d_ctr;   // the called groups; [0..2) the build's counters, [2] the picked calls
        DevBuf<svt_call> d_raw, d_sorted; // the BND calls as emitted / in order
        DevBuf<unsigned long long> d_k, d_k2;   // the order keys of the calls
        DevBuf<uint32_t> d_idx, d_idx2;   // the call indices they carry
        // Not built, nothing allocated.  The caller synchronises first where a launch may still read it.
        void drop() { *this = Bnd{}; }
    } bn;
    // What the last scan ran on (svt_genotype_calls, svt_call_consensus) and its stats: reset when a scan
    // begins, the three set once the index the scan runs on is built.
    struct Last {
        bool merged = false, junction = false;
        uint32_t rearr = 0;               // the scan's rearr mask
        uint32_t bnd = 0;                 // the scan's bnd
        svt_call_bnd_stats bnd_stats{};   // (all zero after bnd = 0)
        svt_call_stats call_stats{};
        svt_call_split_stats split_stats{};
        svt_call_merge_stats merge_stats{};         // (all zero after merge_gap = 0)
        svt_call_junction_stats junction_stats{};   // (all zero after junctions = 0)
        svt_call_rearr_stats rearr_stats{};         // (all zero after rearr = 0)
    } last;
};

// svt_call_consensus's scratch (svt_callseq.inc, svt_callseq_host.inc): nothing allocated before the
// first call on a loaded pileup, gone with the pileup.
struct CallSeqScratch {
    bool ready = false;            // the item table and the reach are those of the loaded pileup
    DevBuf<uint2> d_tab;           // [n_ins] {x, len} per sequence index
    DevBuf<unsigned long long> d_ctr;   // [0] the reach (32 bits), [1..4) the gather's counters
    uint32_t reach = 0;
    svt_call_consensus_stats stats{};
};

// One pool of POA scratch slots (svt_poa.inc, svt_poa_host.inc).
struct PoaPool {
    DevBuf<uint8_t> d;
    uint64_t slot_bytes = 0;
    uint32_t nslots = 0;
};
