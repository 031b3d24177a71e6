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

// svt_call_scan's scratch (svt_call.inc, svt_call_host.inc): nothing allocated before the first scan
// of a loaded pileup, gone with the pileup.
struct CallScratch {
    bool ready = false;
    bool scanned = false;          // svt_call_scan ran on this pileup (svt_genotype_calls)
    uint64_t n_seg = 0;
    DevBuf<uint64_t> d_seg;
    DevBuf<unsigned long long> d_keys, d_tmax, d_tprev;
    DevBuf<uint32_t> d_cid, d_pick;
    DevBuf<uint32_t> d_ctr;        // [0] picked calls, [1] the DEL calls among them, [2..8) events / skipped / big buckets (64 bits each)
    DevBuf<CallAcc> d_acc;
    DevBuf<uint8_t> d_tmp;         // hipcub's temporary storage
    DevBuf<uint8_t> d_flag;        // per cluster: a call
    DevBuf<svt_call> d_calls, d_raw;   // in (chrom, pos, type) order / as emitted
    uint64_t n_calls = 0;
    svt_call_stats stats{};
    // the split by length (len_permille > 0): nothing allocated before the first such scan
    DevBuf<uint32_t> d_first, d_cand, d_kend, d_unit;   // per cluster: first key slot / candidates / their keys' ends / units
    DevBuf<uint8_t> d_cflag;       // per cluster: a candidate
    DevBuf<unsigned long long> d_skeys;   // the candidates' sorted keys
    DevBuf<unsigned long long> d_sctr;    // [0..3) split / groups / big, [3] the candidates (32 bits)
    DevBuf<CallAcc> d_gacc, d_uacc;       // per unit: the groups as accumulated / every unit in order
    svt_call_split_stats split{};
    // the merged index (merge_gap > 0; svt_callmerge.inc, svt_callmerge_host.inc): nothing allocated
    // before the first such scan, rebuilt when (gap, min) change, untouched by svt_reindex
    struct Merged {
        bool built = false;
        uint32_t gap = 0, min_len = 0;    // what it was built for
        DevBuf<uint4> d_ev;               // the merged items, array S's then array I's
        DevBuf<uint32_t> d_off;           // [BA_N][bk_n + 1], rows S and I filled
        uint64_t events[2] = {};          // DEL / INS items
        bool ready = false;               // its own segments (they depend on the extents)
        uint64_t n_seg = 0;
        DevBuf<uint64_t> d_seg;
        svt_call_merge_stats stats{};     // of the build
    } mg;
    bool last_merged = false;             // the last scan ran on the merged index (svt_genotype_calls, svt_call_consensus)
    svt_call_merge_stats merge{};         // the last scan's (all zero after merge_gap = 0)
    // the segment table and the union index (junctions = 1; svt_junction.inc, svt_junction_host.inc):
    // nothing allocated before svt_load_junctions / the first such scan; the index is rebuilt when the
    // table or the base view's (merge_gap, merge_min) change, untouched by svt_reindex
    struct Junction {
        bool loaded = false;              // a table for the loaded pileup (n == 0 included)
        uint64_t n = 0, rows = 0;         // its records and segment rows
        DevBuf<uint64_t> d_toff;          // [n + 1]
        DevBuf<svt_junction_seg> d_tseg;  // [rows]
        bool built = false;
        uint32_t gap = 0, min_len = 0;    // the base view it was built on (gap 0: the plain buckets)
        DevBuf<uint4> d_ev;               // the union's events, array S's then array I's
        DevBuf<uint32_t> d_off;           // [BA_N][bk_n + 1], rows S and I filled
        uint64_t events[2] = {};          // S / I events (the base view's non-items included)
        bool ready = false;               // its own segments (they depend on the extents)
        uint64_t n_seg = 0;
        DevBuf<uint64_t> d_seg;
        svt_call_junction_stats stats{};  // of the build
    } jn;
    bool last_junction = false;           // the last scan ran on the union index (svt_genotype_calls, svt_call_consensus)
    svt_call_junction_stats junction{};   // the last scan's (all zero after junctions = 0)
    // the rearrangement index (rearr != 0; svt_rearr.inc, svt_rearr_host.inc): nothing allocated before the
    // first such scan; rebuilt when the table changes, untouched by svt_reindex
    struct Rearr {
        bool built = false;
        DevBuf<uint4> d_ev;               // the DUP events (row S), then the INV events (row I)
        DevBuf<uint32_t> d_off;           // [BA_N][bk_n + 1], rows S and I filled
        uint64_t events[2] = {};          // DUP / INV items
        bool ready = false;               // its own segments (they depend on the extents)
        uint64_t n_seg = 0;
        DevBuf<uint64_t> d_seg;
        DevBuf<svt_call> d_a, d_b;        // the scan's two sorted lists before their merge: DEL / INS, INV / DUP
        svt_call_rearr_stats stats{};     // of the build
    } rr;
    uint32_t last_rearr = 0;              // the last scan's rearr mask (svt_call_consensus)
    svt_call_rearr_stats rearr{};         // the last scan's (all zero after rearr = 0)
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
