// bam_ingest.cpp -- BGZF/BAM reader -> columnar pileup (svtrek_host.h).
//
// What the reference gets from htslib on this path (refinement.c:114-120) is, per
// yielded record: core.tid, core.pos, core.flag (via bam_endpos, used by the region
// overlap test), n_cigar and the CIGAR -- after bam_read1 has restored a >65535-op
// CIGAR from its CG:B,I tag (htslib bam_tag2cigar) -- plus the two words the soft-clip
// tests read (cigar[n_cigar-1] and cigar[0], which for n_cigar == 0 land in the padded
// read name / the SEQ bytes of htslib's bam1_t data layout).  This reader extracts
// exactly those, once per file, in bounded chunks:
//   1. parallel raw-inflate of the chunk's BGZF blocks (libdeflate if present, else zlib;
//      T threads);
//   2. a sequential scan of the record boundaries (4 bytes per record);
//   3. parallel per-record extraction in two passes (CIGAR lengths incl. CG tags, then
//      copies into the final arrays at prefix-summed offsets).
// A coordinate-sorted BAM (the only kind that has a BAI) needs no reordering; other
// files are stably sorted by (tid, pos) at the end.  SEQ/QUAL/aux are never copied -- except, for
// svth_bam_read_seq, the SEQ bases under every I >= 50 op (the allele-consensus mode's sequences),
// and, for svth_bam_read_sa, the SA:Z values as a segment table.
//
// In reading order: bgzf_scan and ZlibRaw (the one block-header scan, the one zlib inflate of a block);
// BgzfReader (the opened file and its inflated byte stream); parse_header (the one BAM header parse); InsSeq
// and SaTable (the two optional products: size per chunk, extract per record, finish in the final read
// order); Ingest (the read as stages); svth_bam_read_device (compressed batches handed to a device sink).
#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <future>
#include <memory>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "svtrek_host.h"
#include "svt_bamrec.h"

namespace {

using bamrec::rd16;
using bamrec::rd32;

template <typename F>
void parallel_for(int threads, size_t n, F &&f) {   // f(begin, end) over contiguous slices
    const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(threads, 1), n / 4096 + 1));
    if (T == 1) { f((size_t)0, n); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++) th.emplace_back([&, t] { f(n * t / T, n * (t + 1) / T); });
    for (auto &x : th) x.join();
}

// Raw-DEFLATE block decoder: libdeflate when the system has it (libdeflate.so.0, bound at
// run time through its stable C API: alloc / deflate_decompress / free), zlib otherwise.
struct Inflater {
    using alloc_t = void *(*)();
    using dec_t = int (*)(void *, const void *, size_t, void *, size_t, size_t *);
    using free_t = void (*)(void *);
    alloc_t ld_alloc = nullptr;
    dec_t ld_dec = nullptr;
    free_t ld_free = nullptr;
    Inflater() {
        if (getenv("SVTREK_NO_LIBDEFLATE")) return;
        void *h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        ld_alloc = (alloc_t)dlsym(h, "libdeflate_alloc_decompressor");
        ld_dec = (dec_t)dlsym(h, "libdeflate_deflate_decompress");
        ld_free = (free_t)dlsym(h, "libdeflate_free_decompressor");
        if (!ld_alloc || !ld_dec || !ld_free) ld_alloc = nullptr;
    }
    bool fast() const { return ld_alloc != nullptr; }
};
const Inflater &inflater() {
    static const Inflater inf;
    return inf;
}

// Growable array without value-initialisation; large blocks grow by realloc (mremap on
// glibc), so appending a chunk never re-copies or zero-fills what is already there.
template <typename T>
struct RawVec {
    T *p = nullptr;
    size_t n = 0, cap = 0;
    RawVec() = default;
    RawVec(const RawVec &) = delete;
    RawVec &operator=(const RawVec &) = delete;
    ~RawVec() { free(p); }
    bool resize(size_t m) {
        if (m > cap) {
            size_t c = std::max(m, cap + cap / 2 + 1024);
            T *q = (T *)realloc(p, c * sizeof(T));
            if (!q) return false;
            p = q;
            cap = c;
        }
        n = m;
        return true;
    }
    size_t size() const { return n; }
    T *data() { return p; }
    const T *data() const { return p; }
    T &operator[](size_t i) { return p[i]; }
    const T &operator[](size_t i) const { return p[i]; }
    void swap(RawVec &o) { std::swap(p, o.p); std::swap(n, o.n); std::swap(cap, o.cap); }
};

// The window on the inflated byte stream: grown by the host-thread inflate, or (view) pointed at a batch
// buffer that the reader owns -- the device-inflated batches are handed over without a copy.
struct Bytes : RawVec<uint8_t> {
    bool viewed = false;
    ~Bytes() {
        if (viewed) p = nullptr;
    }
    bool resize(size_t m) { return viewed && m > cap ? false : RawVec::resize(m); }   // (a view never grows)
    void view(uint8_t *q, size_t m) {
        if (!viewed) free(p);
        p = q;
        n = cap = m;
        viewed = true;
    }
    void erase_front(size_t k) {
        if (k) memmove(p, p + k, n - k);
        n -= k;
    }
    void clear() { n = 0; }
};

// The BGZF block-header scan (SAM spec 4.1: the gzip magic with FEXTRA, xlen, the BC subfield's BSIZE, the
// trailing ISIZE): the whole blocks of buf[p, n) appended to blks -- coff counted from buf, uoff from u --
// and p, u advanced past them.  Stops in front of a block that is not complete yet.  Returns the error, or
// null; at the end of the file (`eof`) bytes that hold no whole block are an error.
const char *bgzf_scan(const uint8_t *buf, size_t n, bool eof, size_t &p, size_t &u, std::vector<svt_bgzf_block> &blks) {
    while (p + 18 <= n) {
        const uint8_t *h = buf + p;
        if (h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) return "not a BGZF file (bad gzip header)";
        const size_t xlen = rd16(h + 10);
        if (p + 12 + xlen > n) break;
        size_t bsize = 0;
        for (size_t x = 0; x + 4 <= xlen;) {
            const uint8_t *sf = h + 12 + x;
            const size_t slen = rd16(sf + 2);
            if (sf[0] == 66 && sf[1] == 67 && slen == 2) bsize = (size_t)rd16(sf + 4) + 1;
            x += 4 + slen;
        }
        // (a BSIZE smaller than the block's own framing: the deflate length below would wrap)
        if (!bsize || bsize < xlen + 20) return "BGZF block without BC subfield";
        if (p + bsize > n) break;
        blks.push_back(svt_bgzf_block{p + 12 + xlen, u, (uint32_t)(bsize - xlen - 20), rd32(h + bsize - 4)});   // coff, uoff, clen, ulen
        u += blks.back().ulen;
        p += bsize;
    }
    return eof && blks.empty() && n ? "truncated BGZF block at end of file" : nullptr;
}

// Raw inflate of one BGZF block with zlib, the stream reused from block to block.
struct ZlibRaw {
    z_stream zs;
    bool ok;
    ZlibRaw() {
        memset(&zs, 0, sizeof zs);
        ok = inflateInit2(&zs, -15) == Z_OK;
    }
    ZlibRaw(const ZlibRaw &) = delete;
    ~ZlibRaw() {
        if (ok) inflateEnd(&zs);
    }
    bool block(const uint8_t *in, size_t clen, uint8_t *out, size_t ulen) {
        if (!ok) return false;
        inflateReset(&zs);
        zs.next_in = const_cast<uint8_t *>(in);
        zs.avail_in = (uInt)clen;
        zs.next_out = out;
        zs.avail_out = (uInt)ulen;
        return inflate(&zs, Z_FINISH) == Z_STREAM_END && zs.total_out == ulen;
    }
};

// The opened BAM and its inflated byte stream.  The file is closed when the reader goes, after the helper
// thread that reads it has finished; no caller closes it or waits for that thread by hand.
struct BgzfReader {
    FILE *f = nullptr;             // null: the file did not open
    int threads = 1;               // (clamped to >= 1)
    std::vector<uint8_t> comp;     // compressed bytes not yet consumed
    bool eof = false;
    std::string err;
    // device inflate (svth_inflater): batches of ~`batch` compressed bytes, read with parallel
    // preads into a reused input buffer and inflated by inf->inflate into one of two reused
    // output buffers (from inf->alloc: pinned host memory, so the copies to and from the device
    // run at full speed); the next batch is read and inflated by a helper thread while the
    // caller parses the current one
    svth_inflater cfg{};                   // (the caller's, copied)
    const svth_inflater *inf = nullptr;    // &cfg, or null: host threads inflate
    static constexpr size_t HEAD = 64ull << 20;   // room in front of a batch for the previous one's tail
    struct Buf {
        uint8_t *p = nullptr;
        size_t cap = 0;
        bool pinned = false;   // from inf->alloc (else malloc: pinned memory was refused)
    };
    Buf cins[2], outs[2];  // compressed input (one inflated, one being read); output (one parsed, one filled)
    size_t cin_n[2] = {0, 0};
    int read_i = 0, fill_i = 0;   // the input / output buffer the next batch goes to
    // the partial block at the end of the last batch read: cins[carry_i][carry_p, +carry_n)
    int carry_i = 0;
    size_t carry_p = 0, carry_n = 0;
    struct Comp {                 // a batch read and scanned: its blocks in cins[i][0, p)
        int i = 0;
        size_t p = 0, u = 0;
        std::vector<svt_bgzf_block> blks;
        bool ok = false;
        std::string err;
    };
    std::future<Comp> pending_comp;
    uint64_t foff = 0, fsize = 0;
    struct Batch {
        uint8_t *p = nullptr;   // outs[i].p: HEAD bytes, then n inflated bytes
        size_t n = 0;
        bool ok = false;
        std::string err;
    };
    std::future<Batch> pending;
    // stage times (s): read, header scan, buffer allocation (reader, inflater), inflate, parser
    // waiting on a batch
    double t_read = 0, t_scan = 0, t_alloc_r = 0, t_alloc = 0, t_inflate = 0, t_wait = 0;
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

    BgzfReader(const char *path, int threads_, const svth_inflater *inf_) : threads(threads_ < 1 ? 1 : threads_) {
        if (inf_) {
            cfg = *inf_;
            inf = &cfg;
        }
        f = fopen(path, "rb");
        struct stat st;
        if (f) fsize = fstat(fileno(f), &st) == 0 ? (uint64_t)st.st_size : 0;
    }
    BgzfReader(const BgzfReader &) = delete;
    BgzfReader &operator=(const BgzfReader &) = delete;
    ~BgzfReader() {
        drop_pending();   // (the helper thread reads f)
        for (Buf *b : {&cins[0], &cins[1], &outs[0], &outs[1]}) release(*b);
        if (f) fclose(f);
    }
    // The message of a failed read: the reader's own when it has one (once the helper thread, which may be
    // the one that set it, has finished), else m.
    std::string error(const std::string &m) {
        drop_pending();
        return err.empty() ? m : err;
    }
    void drop_pending() {
        if (pending.valid()) (void)pending.get();
        if (pending_comp.valid()) (void)pending_comp.get();
    }
    void release(Buf &b) {
        if (b.p) {
            if (b.pinned) inf->release(inf->user, b.p);
            else free(b.p);
        }
        b = Buf{};
    }
    // grow to >= need, keeping the first `keep` bytes; pinned memory when the inflater offers it,
    // pageable memory when pinning is refused (the copies are only slower)
    bool reserve(Buf &b, size_t need, size_t keep) {
        if (need <= b.cap) return true;
        const size_t c = std::max(need, b.cap + b.cap / 2);
        bool pinned = inf && inf->alloc && inf->release;
        uint8_t *q = pinned ? (uint8_t *)inf->alloc(inf->user, c) : nullptr;
        if (!q) {
            pinned = false;
            q = (uint8_t *)malloc(c);
        }
        if (!q) return false;
        if (keep) memcpy(q, b.p, keep);
        release(b);
        b.p = q;
        b.cap = c;
        b.pinned = pinned;
        return true;
    }

    // Continue at compressed file offset `coff` (a BGZF block start).
    bool seek(uint64_t coff) {
        drop_pending();
        comp.clear();
        cin_n[0] = cin_n[1] = 0;
        carry_n = 0;
        foff = coff;
        eof = false;
        if (fseeko(f, (off_t)coff, SEEK_SET) != 0) { err = "cannot seek in BAM (BAI offset past the end?)"; return false; }
        return true;
    }

    // Append the next ~want compressed bytes to buffer b (holding n), `threads` preads at once.
    bool read_batch(Buf &b, size_t &n, size_t want) {
        if (foff >= fsize) { eof = true; return true; }
        want = (size_t)std::min<uint64_t>(want, fsize - foff);
        const double t0 = now();
        if (!reserve(b, n + want + 64, n)) { err = "out of host memory"; return false; }
        const double t1 = now();
        t_alloc_r += t1 - t0;
        const int fd = fileno(f);
        std::atomic<int> bad{0};
        uint8_t *dst = b.p + n;
        const uint64_t at = foff;
        parallel_for(threads, want, [&](size_t a, size_t e) {
            for (size_t o = a; o < e;) {
                const ssize_t r = pread(fd, dst + o, e - o, (off_t)(at + o));
                if (r <= 0) { bad = 1; return; }
                o += (size_t)r;
            }
        });
        t_read += now() - t1;
        if (bad) { err = "cannot read BAM"; return false; }
        n += want;
        foff += want;
        if (foff >= fsize) eof = true;
        return true;
    }

    // Read and scan the next batch into cins[read_i] (the previous batch's partial block first).
    Comp read_next() {
        Comp c;
        c.i = read_i;
        Buf &b = cins[read_i];
        size_t &n = cin_n[read_i];
        const size_t want = inf->batch_bytes ? inf->batch_bytes : (1ull << 30);
        n = 0;
        if (carry_n) {
            const double t0 = now();
            if (!reserve(b, carry_n + want + 64, 0)) { c.err = "out of host memory"; return c; }
            t_alloc_r += now() - t0;
            memcpy(b.p, cins[carry_i].p + carry_p, carry_n);
            n = carry_n;
        }
        size_t p = 0, u = 0;
        for (;;) {
            if (!eof && !read_batch(b, n, want)) { c.err = err; return c; }
            const double ts = now();
            const char *e = bgzf_scan(b.p, n, eof, p, u, c.blks);
            t_scan += now() - ts;
            if (e) { c.err = e; return c; }
            if (!c.blks.empty() || eof) break;   // (else a single block larger than what was read so far)
        }
        c.p = p;
        c.u = u;
        c.ok = true;
        carry_i = read_i;
        carry_p = p;
        carry_n = n - p;
        read_i ^= 1;
        return c;
    }

    // Inflate the next batch (helper thread), the batch after it being read meanwhile; ok && n ==
    // 0 at end of file.
    Batch produce() {
        Batch b;
        Comp c = pending_comp.valid() ? pending_comp.get() : read_next();
        // a batch of empty blocks only (ISIZE 0 each) is skipped, not taken for the end of file
        while (c.ok && !c.blks.empty() && c.u == 0) {
            if (eof && !carry_n) { c.blks.clear(); break; }
            c = read_next();
        }
        if (!c.ok) { b.err = c.err; return b; }
        if (c.blks.empty()) { b.ok = true; return b; }   // end of file
        if (!eof || carry_n) pending_comp = std::async(std::launch::async, [this] { return read_next(); });
        Buf &o = outs[fill_i];
        double t0 = now();
        if (!reserve(o, HEAD + c.u + 16, 0)) { b.err = "out of host memory"; return b; }
        double t1 = now();
        t_alloc += t1 - t0;
        char e[256] = {0};
        const int rc = inf->inflate(inf->user, cins[c.i].p, c.p, c.blks.data(), c.blks.size(), o.p + HEAD, c.u, e, sizeof e);
        t_inflate += now() - t1;
        if (rc != 0) {
            b.err = e[0] ? e : "BGZF inflate failed";
            return b;
        }
        b.p = o.p;
        b.n = c.u;
        b.ok = true;
        fill_i ^= 1;
        return b;
    }

    // Device path of next(): the pending batch (or a synchronous first one) becomes the buffer,
    // the unconsumed tail [at, size) moved in front of it; the batch after it starts, into the
    // output buffer the parser just left.
    bool next_device(Bytes &out, size_t &at) {
        const double tw = now();
        Batch b = pending.valid() ? pending.get() : produce();
        t_wait += now() - tw;
        if (!b.ok) { err = b.err; return false; }
        if (b.n == 0) return false;   // end of file
        const size_t tail = out.size() - at;
        if (tail > HEAD) { err = "a BAM record longer than 64 MiB"; return false; }
        memcpy(b.p + HEAD - tail, out.data() + at, tail);
        out.view(b.p, HEAD + b.n);   // (the reader owns the buffer)
        at = HEAD - tail;
        pending = std::async(std::launch::async, [this] { return produce(); });
        return true;
    }

    // Make more inflated bytes available in out (consumed up to `at`); false at end of file /
    // on error.
    bool next(Bytes &out, size_t &at) {
        if (inf) return next_device(out, at);
        if (at) {
            out.erase_front(at);
            at = 0;
        }
        const size_t CHUNK = 64u << 20;
        std::vector<svt_bgzf_block> blks;
        size_t p = 0, u = 0;
        while (blks.empty()) {
            if (!eof) {
                size_t old = comp.size();
                comp.resize(old + CHUNK);
                size_t got = fread(comp.data() + old, 1, CHUNK, f);
                comp.resize(old + got);
                if (got < CHUNK) eof = true;
            }
            if (comp.empty()) return false;   // end of file
            if (const char *e = bgzf_scan(comp.data(), comp.size(), eof, p, u, blks)) { err = e; return false; }
            // (no block yet and not at the end: a single block larger than what was read so far)
        }
        const size_t base = out.size();
        if (!out.resize(base + u)) { err = "out of host memory"; return false; }
        if (!inflate_host(blks, out.data() + base)) { err = "corrupt BGZF block (inflate failed)"; return false; }
        comp.erase(comp.begin(), comp.begin() + (ptrdiff_t)p);
        return true;
    }

    // Host threads: the blocks of comp raw-inflated to dst + uoff (libdeflate when present, else zlib).
    bool inflate_host(const std::vector<svt_bgzf_block> &blks, uint8_t *dst) {
        std::atomic<int> bad{0};
        const Inflater &dec = inflater();
        parallel_for(threads, blks.size() * 4096, [&](size_t b0, size_t b1) {
            if (dec.fast()) {
                void *d = dec.ld_alloc();
                if (!d) { bad = 1; return; }
                for (size_t i = b0 / 4096; i < b1 / 4096; i++) {
                    const svt_bgzf_block &k = blks[i];
                    size_t got = 0;
                    if (dec.ld_dec(d, comp.data() + k.coff, k.clen, dst + k.uoff, k.ulen, &got) != 0 || got != k.ulen) bad = 1;
                }
                dec.ld_free(d);
                return;
            }
            ZlibRaw z;
            for (size_t i = b0 / 4096; i < b1 / 4096; i++)
                if (!z.block(comp.data() + blks[i].coff, blks[i].clen, dst + blks[i].uoff, blks[i].ulen)) bad = 1;
        });
        return !bad;
    }
};

// The BAI's linear index (SAM spec 5.2): per contig, the smallest virtual offset of the
// records overlapping each 16 kb window.  Bins are skipped: a coordinate-sorted file read
// from the linear-index offset reaches every record a region query can yield.
struct BaiLinear {
    std::vector<std::vector<uint64_t>> ioff;
    bool load(const std::string &path, std::string &err) {
        FILE *f = fopen(path.c_str(), "rb");
        if (!f) { err = "cannot open BAI: " + path; return false; }
        auto rd = [&](void *p, size_t n) { return fread(p, 1, n, f) == n; };
        char magic[4];
        int32_t n_ref = 0;
        bool ok = rd(magic, 4) && memcmp(magic, "BAI\1", 4) == 0 && rd(&n_ref, 4) && n_ref >= 0;
        if (ok) ioff.resize((size_t)n_ref);
        for (int32_t r = 0; ok && r < n_ref; r++) {
            int32_t n_bin = 0;
            ok = rd(&n_bin, 4) && n_bin >= 0;
            for (int32_t i = 0; ok && i < n_bin; i++) {
                uint32_t bin;
                int32_t n_chunk;
                ok = rd(&bin, 4) && rd(&n_chunk, 4) && n_chunk >= 0 && fseeko(f, 16 * (off_t)n_chunk, SEEK_CUR) == 0;
            }
            int32_t n_intv = 0;
            ok = ok && rd(&n_intv, 4) && n_intv >= 0;
            if (ok) {
                ioff[(size_t)r].resize((size_t)n_intv);
                ok = n_intv == 0 || rd(ioff[(size_t)r].data(), 8 * (size_t)n_intv);
            }
        }
        fclose(f);
        if (!ok) err = "corrupt BAI: " + path;
        return ok;
    }
    // Where a read of the records from (tid, beg) on starts; false = no such record.  A zero
    // entry is a window no record overlapped (older indexers leave those 0 instead of the next
    // window's offset): virtual offset 0 is the BAM header, never a record, so the next
    // non-zero entry -- of this contig or a later one -- is taken instead.
    bool start(int32_t tid, int64_t beg, uint64_t &voff) const {
        for (size_t t = (size_t)std::max(tid, 0); t < ioff.size(); t++) {
            const int64_t w = (int32_t)t == tid ? std::max<int64_t>(beg, 0) >> 14 : 0;
            for (size_t k = (size_t)std::max<int64_t>(w, 0); k < ioff[t].size(); k++)
                if (ioff[t][k] != 0) { voff = ioff[t][k]; return true; }
        }
        return false;
    }
};

}  // namespace

struct svth_bam {
    std::vector<std::string> names;
    std::vector<int64_t> tid_off;
    RawVec<int32_t> pos, endpos;
    RawVec<uint64_t> cig_off;
    RawVec<uint32_t> cigar;
    RawVec<uint8_t> clip;
    int64_t n_records = 0, n_cg = 0;
    // svth_bam_read_seq: the inserted bases of the kept reads' I >= 50 ops, in (read, op) order
    bool has_seq = false;
    RawVec<uint32_t> ins_cnt, ins_len;   // per read its I >= 50 ops; per op its length
    RawVec<uint64_t> ins_off;            // [n_ins + 1]
    RawVec<uint8_t> ins_bases;           // nt4 codes
    // svth_bam_read_sa: the segment table of the kept reads that carry an SA:Z tag (include/svtrek_junction.h)
    bool has_sa = false;
    std::vector<uint64_t> sa_read, sa_off;   // sorted pileup read indices; [n + 1] rows
    std::vector<svt_junction_seg> sa_seg;
    int64_t n_sa_malformed = 0;          // records whose SA value did not parse (their row is dropped)
    double stage_s[6] = {0, 0, 0, 0, 0, 0};   // read, scan, alloc, inflate, wait, total
};

namespace {

constexpr uint32_t OP_I = 1, INS_MIN = 50;   // the I ops that carry a sequence (include/svtrek_gpu.h: I >= 50)

// A record's I >= 50 ops: their count and the sum of their lengths.
inline void ins_census(const bamrec::View &v, uint64_t &cnt, uint64_t &bases) {
    cnt = 0;
    bases = 0;
    for (uint32_t j = 0; j < v.n; j++) {
        const uint32_t w = bamrec::rd32(v.cig + 4ull * j);
        if ((w & 0xfu) == OP_I && (w >> 4) >= INS_MIN) { cnt++; bases += w >> 4; }
    }
}

// Where a record's SEQ and aux fields start (r: the record after its block_size word), behind the name and the
// stored CIGAR (the placeholder, when the CIGAR itself sits in a CG tag).  aux is null for l_seq < 0.
struct SeqAux { const uint8_t *seq, *aux; int64_t l_seq; };
inline SeqAux seq_aux(const uint8_t *r) {
    const int64_t l_seq = (int32_t)rd32(r + 16);
    const uint8_t *seq = r + 32 + r[8] + 4ull * rd16(r + 12);
    return {seq, l_seq < 0 ? nullptr : seq + (size_t)(l_seq + 1) / 2 + (size_t)l_seq, l_seq};
}

// The lengths and bases of those ops (r: the record after its block_size word, bs: that word).  The
// query offset of an op is the summed length of the M, I, S, = and X ops before it in the CIGAR the
// pileup keeps (the CG-restored one included); bases come from the 4-bit SEQ, high nibble first, codes
// 1, 2, 4, 8 -> 0 .. 3 and every other code -> 4.  An op that runs past l_seq (l_seq == 0: every op, or
// a SEQ that runs past the record) keeps its CIGAR length with every base 4.
inline void ins_extract(const bamrec::View &v, const uint8_t *r, uint32_t bs, uint32_t *len_out, uint8_t *base_out) {
    static const uint8_t NT4[16] = {4, 0, 1, 4, 2, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4};
    const SeqAux sa = seq_aux(r);
    const uint8_t *seq = sa.seq;
    const int64_t l_seq = sa.l_seq < 0 || seq + (size_t)(sa.l_seq + 1) / 2 > r + bs ? 0 : sa.l_seq;
    uint64_t q = 0;
    for (uint32_t j = 0; j < v.n; j++) {
        const uint32_t w = bamrec::rd32(v.cig + 4ull * j), op = w & 0xfu, len = w >> 4;
        if (op == OP_I && len >= INS_MIN) {
            *len_out++ = len;
            if (q + len <= (uint64_t)l_seq)
                for (uint64_t t = q; t < q + len; t++) *base_out++ = NT4[(seq[t >> 1] >> ((t & 1) ? 0 : 4)) & 0xf];
            else {
                memset(base_out, 4, len);
                base_out += len;
            }
        }
        if (op == bamrec::OP_M || op == OP_I || op == bamrec::OP_S || op == bamrec::OP_EQ || op == bamrec::OP_X) q += len;
    }
}

// The value of the record's SA:Z tag (r: the record after its block_size word, bs: that word), found by
// walking the aux fields as the CG restoration does: [*beg, *end) without the NUL.  False: no such tag
// (or aux fields that cannot be walked).
inline bool find_sa(const uint8_t *r, uint32_t bs, const uint8_t **beg, const uint8_t **vend) {
    const uint8_t *end = r + bs;
    const uint8_t *p = seq_aux(r).aux;
    if (!p) return false;
    while (p < end && end - p >= 3) {
        const char t0 = (char)p[0], t1 = (char)p[1], ty = (char)p[2];
        p += 3;
        size_t sz = 0;
        switch (ty) {
        case 'A': case 'c': case 'C': sz = 1; break;
        case 's': case 'S': sz = 2; break;
        case 'i': case 'I': case 'f': sz = 4; break;
        case 'Z': case 'H': {
            const uint8_t *q = p;
            while (q < end && *q) q++;
            if (q >= end) return false;
            if (ty == 'Z' && t0 == 'S' && t1 == 'A') { *beg = p; *vend = q; return true; }
            p = q + 1;
            continue;
        }
        case 'B': {
            if (end - p < 5) return false;
            const char sub = (char)p[0];
            const uint64_t n = bamrec::rd32(p + 1);
            const size_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2
                              : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
            if (!es || (uint64_t)(end - p - 5) < n * es) return false;
            p += 5 + n * es;
            continue;
        }
        default:
            return false;
        }
        if ((size_t)(end - p) < sz) return false;
        p += sz;
    }
    return false;
}

// One CIGAR as a segment's numbers: cl / ct the leading / trailing run of S and H, qlen the M I = X, rlen
// the M D N = X (include/svtrek_junction.h).  False when a sum passes 32 bits.
struct SegLen { uint64_t cl = 0, ct = 0, qlen = 0, rlen = 0; bool lead = true; };
inline void seg_op(SegLen &g, uint32_t op, uint64_t len) {
    const bool clip = op == bamrec::OP_S || op == 5u;
    if (clip) { if (g.lead) g.cl += len; g.ct += len; }
    else { g.lead = false; g.ct = 0; }
    if (op == bamrec::OP_M || op == OP_I || op == bamrec::OP_EQ || op == bamrec::OP_X) g.qlen += len;
    if (op == bamrec::OP_M || op == bamrec::OP_D || op == bamrec::OP_N || op == bamrec::OP_EQ || op == bamrec::OP_X) g.rlen += len;
}
inline bool seg_make(const SegLen &g, int32_t tid, uint32_t strand, uint64_t r_beg, svt_junction_seg *out) {
    const uint64_t qb = strand ? g.ct : g.cl;
    if (r_beg + g.rlen > 0xffffffffull || qb + g.qlen > 0xffffffffull) return false;
    *out = svt_junction_seg{tid, strand, (uint32_t)r_beg, (uint32_t)(r_beg + g.rlen), (uint32_t)qb, (uint32_t)(qb + g.qlen)};
    return true;
}

// The entries rname,pos,strand,CIGAR,mapQ,NM; of an SA value appended to `out`.  False -- a malformed
// value -- for a missing or empty field, an unknown rname, an empty or invalid CIGAR, pos < 1 (or past
// 2^31 - 1), a strand other than + / -, or an entry without its terminator.
bool parse_sa(const uint8_t *p, const uint8_t *end, const std::unordered_map<std::string, int32_t> &tids,
              std::vector<svt_junction_seg> &out) {
    while (p < end) {
        const uint8_t *semi = (const uint8_t *)memchr(p, ';', (size_t)(end - p));
        if (!semi) return false;
        const uint8_t *f[7];
        int nf = 0;
        f[nf++] = p;
        for (const uint8_t *q = p; q < semi; q++)
            if (*q == ',') {
                if (nf == 6) return false;
                f[nf++] = q + 1;
            }
        if (nf != 6) return false;
        f[6] = semi + 1;
        for (int k = 0; k < 6; k++)
            if (f[k + 1] - f[k] < 2) return false;   // (an empty field: only its separator)
        const auto it = tids.find(std::string((const char *)f[0], (size_t)(f[1] - f[0] - 1)));
        if (it == tids.end()) return false;
        uint64_t pos = 0;
        for (const uint8_t *q = f[1]; q < f[2] - 1; q++) {
            if (*q < '0' || *q > '9' || pos > 0x7fffffffull) return false;
            pos = pos * 10 + (uint64_t)(*q - '0');
        }
        if (pos < 1 || pos > 0x7fffffffull) return false;
        if (f[3] - f[2] != 2 || (*f[2] != '+' && *f[2] != '-')) return false;
        SegLen g;
        uint64_t len = 0;
        bool digits = false;
        for (const uint8_t *q = f[3]; q < f[4] - 1; q++) {
            if (*q >= '0' && *q <= '9') {
                len = len * 10 + (uint64_t)(*q - '0');
                digits = true;
                if (len > 0xfffffffull) return false;
            } else {
                static const char OPS[] = "MIDNSHP=X";
                const char *o = (const char *)memchr(OPS, *q, 9);
                if (!o || !digits) return false;
                seg_op(g, (uint32_t)(o - OPS), len);
                len = 0;
                digits = false;
            }
        }
        if (digits) return false;                     // (a length without its op)
        for (int k = 4; k < 6; k++)                   // mapQ and NM: numbers, not otherwise read
            for (const uint8_t *q = f[k]; q < f[k + 1] - 1; q++)
                if (*q < '0' || *q > '9') return false;
        svt_junction_seg sg;
        if (!seg_make(g, it->second, *f[2] == '-' ? 1u : 0u, pos - 1, &sg)) return false;
        out.push_back(sg);
        p = semi + 1;
    }
    return true;
}

// The BAM header (SAM spec 4.2: magic, text, n_ref, the reference list) read through take(k): "make k more
// bytes available at the cursor, hand them out and move past them" (null: there are no more).  Returns the
// error, or an empty string; `suffix` ends the two messages about a header that stops early.
template <typename Take>
std::string parse_header(Take &&take, const char *suffix, int32_t &n_ref, std::vector<std::string> *names) {
    const uint8_t *p = take(8);
    if (!p || memcmp(p, "BAM\1", 4) != 0) return "not a BAM file";
    const size_t l_text = rd32(p + 4);
    if (!(p = take(l_text + 4))) return std::string("truncated BAM header") + suffix;
    n_ref = (int32_t)rd32(p + l_text);
    if (n_ref < 0) return "bad n_ref";
    for (int32_t i = 0; i < n_ref; i++) {
        const size_t ln = (p = take(4)) ? rd32(p) : 0;
        if (!p || !(p = take(ln + 4))) return std::string("truncated reference list") + suffix;
        if (names) names->emplace_back((const char *)p, ln ? ln - 1 : 0);
    }
    return {};
}

// One chunk of whole records in the inflated buffer: what the two passes over it share.
struct Chunk {
    const uint8_t *buf = nullptr;     // roff counts from here
    std::vector<size_t> roff;         // each record, after its block_size word
    std::vector<bamrec::View> views;
    std::vector<size_t> slot;         // its index among the kept reads of the file ((size_t)-1: not kept)
    std::vector<uint64_t> off;        // [nr + 1] its CIGAR's place in the chunk's share of the arena
    size_t nr = 0, end = 0;           // the records taken; the buffer offset behind them
    const uint8_t *rec(size_t i) const { return buf + roff[i]; }
    uint32_t bs(size_t i) const { return rd32(buf + roff[i] - 4); }
};

// The reads of `v` in the order idx.
template <typename T>
bool permute(RawVec<T> &v, const std::vector<size_t> &idx) {
    RawVec<T> w;
    if (!w.resize(idx.size())) return false;
    for (size_t k = 0; k < idx.size(); k++) w[k] = v[idx[k]];
    v.swap(w);
    return true;
}

// Rows of varying length -- row i is data[off[i], off[i + 1]) -- in the order idx.
template <typename T>
bool permute_rows(RawVec<uint64_t> &off, RawVec<T> &data, const std::vector<size_t> &idx) {
    RawVec<uint64_t> off2;
    RawVec<T> data2;
    if (!off2.resize(idx.size() + 1) || !data2.resize(data.size())) return false;
    uint64_t w = 0;
    for (size_t k = 0; k < idx.size(); k++) {
        const uint64_t o = off[idx[k]], m = off[idx[k] + 1] - o;
        off2[k] = w;
        if (m) memcpy(data2.data() + w, data.data() + o, sizeof(T) * m);
        w += m;
    }
    off2[idx.size()] = w;
    off.swap(off2);
    data.swap(data2);
    return true;
}

// svth_bam_read_seq's product: the inserted bases of the kept reads' I >= 50 ops, in (read, op) order.
struct InsSeq {
    svth_bam &b;
    std::vector<uint64_t> ioff, iboff;   // [nr + 1] where the ops / the bases of each record of the chunk go
    explicit InsSeq(svth_bam &b_) : b(b_) {}

    // Before the parallel copy: the census of the chunk and room for its ops and bases; false: out of memory.
    bool size(const Chunk &c, int threads) {
        ioff.assign(c.nr + 1, 0);
        iboff.assign(c.nr + 1, 0);
        parallel_for(threads, c.nr, [&](size_t i0, size_t i1) {
            for (size_t i = i0; i < i1; i++)
                if (c.views[i].ok) ins_census(c.views[i], ioff[i + 1], iboff[i + 1]);
        });
        ioff[0] = b.ins_len.size();
        iboff[0] = b.ins_bases.size();
        for (size_t i = 0; i < c.nr; i++) {
            ioff[i + 1] += ioff[i];
            iboff[i + 1] += iboff[i];
        }
        return b.ins_cnt.resize(b.pos.size()) && b.ins_len.resize(ioff[c.nr]) && b.ins_bases.resize(iboff[c.nr]);
    }
    // Inside it, for a kept record.
    void extract(const Chunk &c, size_t i) {
        const uint64_t cnt = ioff[i + 1] - ioff[i];
        b.ins_cnt[c.slot[i]] = (uint32_t)cnt;
        if (cnt) ins_extract(c.views[i], c.rec(i), c.bs(i), b.ins_len.data() + ioff[i], b.ins_bases.data() + iboff[i]);
    }
    // The ops' offsets, and the bases, in the final (read, op) order: idx is the reads' reorder (empty: none).
    bool finish(const std::vector<size_t> &idx) {
        if (!idx.empty()) {   // per file-order read its first op and first base, then both in the reads' final order
            const size_t n = idx.size();
            RawVec<uint64_t> first, fbase;
            if (!first.resize(n + 1) || !fbase.resize(n + 1)) return false;
            first[0] = fbase[0] = 0;
            for (size_t i = 0, k = 0; i < n; i++) {
                first[i + 1] = first[i] + b.ins_cnt[i];
                fbase[i + 1] = fbase[i];
                for (; k < first[i + 1]; k++) fbase[i + 1] += b.ins_len[k];
            }
            if (!permute_rows(fbase, b.ins_bases, idx) || !permute_rows(first, b.ins_len, idx)) return false;
        }
        if (!b.ins_off.resize(b.ins_len.size() + 1)) return false;
        b.ins_off[0] = 0;
        for (size_t k = 0; k < b.ins_len.size(); k++) b.ins_off[k + 1] = b.ins_off[k] + b.ins_len[k];
        b.has_seq = true;
        return true;
    }
};

// svth_bam_read_sa's product: the segment table of the kept reads that carry an SA:Z tag.
struct SaTable {
    svth_bam &b;
    std::unordered_map<std::string, int32_t> tids;
    // per record of the chunk its rows (the own segment first; empty: no SA tag, or a malformed one)
    std::vector<std::vector<svt_junction_seg>> rows;
    std::vector<uint8_t> bad;
    explicit SaTable(svth_bam &b_) : b(b_) {}

    void names() {
        b.sa_off.assign(1, 0);
        for (size_t t = 0; t < b.names.size(); t++) tids.emplace(b.names[t], (int32_t)t);   // (the first of equal names)
    }
    // Before the parallel copy.
    void size(const Chunk &c) {
        rows.assign(c.nr, {});
        bad.assign(c.nr, 0);
    }
    // Inside it, for a kept record.
    void extract(const Chunk &c, size_t i) {
        const bamrec::View &v = c.views[i];
        const uint8_t *sa0, *sa1;
        if (!find_sa(c.rec(i), c.bs(i), &sa0, &sa1)) return;
        SegLen g;
        for (uint32_t j = 0; j < v.n; j++) {
            const uint32_t w = rd32(v.cig + 4ull * j);
            seg_op(g, w & 0xfu, w >> 4);
        }
        if (v.flag & 4u) g.rlen = 0;   // (bam_endpos: an unmapped record covers no reference base)
        rows[i].resize(1);
        if (!seg_make(g, v.tid, (v.flag >> 4) & 1u, (uint64_t)v.pos, &rows[i][0]) || !parse_sa(sa0, sa1, tids, rows[i])) {
            rows[i].clear();
            bad[i] = 1;
        }
    }
    // Behind it: the chunk's rows appended to the table, in file order.
    void collect(const Chunk &c) {
        for (size_t i = 0; i < c.nr; i++) {
            b.n_sa_malformed += bad[i];
            if (rows[i].empty()) continue;
            b.sa_read.push_back(c.slot[i]);
            b.sa_seg.insert(b.sa_seg.end(), rows[i].begin(), rows[i].end());
            b.sa_off.push_back(b.sa_seg.size());
        }
    }
    // The table in the final read order, `read` holding final indices: idx is the reads' reorder (empty: none).
    void finish(const std::vector<size_t> &idx) {
        b.has_sa = true;
        if (idx.empty()) return;
        std::vector<uint64_t> inv(idx.size()), read, off(1, 0);
        std::vector<svt_junction_seg> seg;
        for (size_t k = 0; k < idx.size(); k++) inv[idx[k]] = k;
        std::vector<size_t> ord(b.sa_read.size());
        std::iota(ord.begin(), ord.end(), 0);
        std::sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return inv[b.sa_read[x]] < inv[b.sa_read[y]]; });
        for (size_t j : ord) {
            read.push_back(inv[(size_t)b.sa_read[j]]);
            seg.insert(seg.end(), b.sa_seg.begin() + (ptrdiff_t)b.sa_off[j], b.sa_seg.begin() + (ptrdiff_t)b.sa_off[j + 1]);
            off.push_back(seg.size());
        }
        b.sa_read.swap(read);
        b.sa_off.swap(off);
        b.sa_seg.swap(seg);
    }
};

constexpr int WANT_SEQ = 1, WANT_SA = 2;

// One read of a BAM into a svth_bam, as stages.  A stage that fails leaves its message in err and returns
// false; the pileup, the file and the buffers go with the Ingest.
struct Ingest {
    BgzfReader rd;
    const int want;                  // WANT_* bits
    const bool region;               // a read up to (tid1, end1); `done` once that is reached
    const int32_t tid1;
    const int64_t end1;
    std::unique_ptr<svth_bam> b{new svth_bam()};
    InsSeq ins{*b};
    SaTable sa{*b};
    Bytes buf;                       // inflated bytes, consumed up to `at`
    size_t at = 0;
    int32_t n_ref = 0;
    RawVec<int32_t> tid_of;          // per kept read
    uint64_t narena = 0;             // CIGAR words kept so far
    bool done = false;
    std::string err;

    Ingest(const char *path, int threads, const svth_inflater *inf, int want_, bool region_, int32_t tid1_, int64_t end1_)
        : rd(path, threads, inf), want(want_), region(region_), tid1(tid1_), end1(end1_) {}

    bool fail(const char *m) { err = m; return false; }
    bool need(size_t k) {
        while (buf.size() - at < k)
            if (!rd.next(buf, at)) return false;
        return true;
    }

    bool header() {
        err = parse_header([&](size_t k) -> const uint8_t * {
            if (!need(k)) return nullptr;
            at += k;
            return buf.data() + at - k;
        }, "", n_ref, &b->names);
        if (err.empty() && (want & WANT_SA)) sa.names();
        return err.empty();
    }

    // A region read continues at the BAI's linear-index offset of (tid0, beg0).
    bool seek_region(const char *path, int32_t tid0, int64_t beg0) {
        if (!region) return true;
        BaiLinear bai;
        if (!bai.load(std::string(path) + ".bai", err)) return false;
        uint64_t voff = 0;
        if (!bai.start(tid0, beg0, voff)) {   // no record at or after the region start
            done = true;
            return true;
        }
        if (!rd.seek(voff >> 16)) return fail("cannot seek in BAM");
        buf.clear();
        at = 0;
        const size_t uo = (size_t)(voff & 0xffff);
        if (uo && !need(uo)) return fail("BAI offset past the end of the BAM");
        at += uo;
        return true;
    }

    // The sequential boundary scan over the complete records in the buffer.  None (c.nr == 0): one record
    // larger than the buffer, which was read on.
    bool scan(Chunk &c) {
        c.roff.clear();
        size_t p = at;
        while (buf.size() - p >= 4) {
            const uint32_t bs = rd32(buf.data() + p);
            if (bs < 32) return fail("corrupt BAM record (block_size < 32)");
            if (buf.size() - p < 4 + (size_t)bs) break;
            c.roff.push_back(p + 4);
            p += 4 + bs;
        }
        if (c.roff.empty() && !need(4 + (size_t)rd32(buf.data() + at))) return fail("truncated BAM record");
        c.buf = buf.data();
        c.nr = c.roff.size();
        c.end = p;
        return true;
    }

    // Pass 1 (parallel): every record's CIGAR located; then the region cut: in a sorted file the first record
    // past (tid1, end1) ends the read.
    void view(Chunk &c) {
        c.views.resize(c.nr);
        parallel_for(rd.threads, c.nr, [&](size_t i0, size_t i1) {
            for (size_t i = i0; i < i1; i++) c.views[i] = bamrec::view(c.rec(i), c.bs(i), n_ref);
        });
        if (!region) return;
        for (size_t i = 0; i < c.nr; i++) {
            const int32_t t = (int32_t)rd32(c.rec(i)), ps = (int32_t)rd32(c.rec(i) + 4);
            if (t < 0 || t > tid1 || (t == tid1 && (int64_t)ps >= end1)) {
                c.nr = i;
                c.end = c.roff[i] - 4;
                done = true;
                break;
            }
        }
    }

    // Where every record of the chunk goes (prefix offsets), and room for it in the columns and products.
    bool layout(Chunk &c) {
        size_t k = b->pos.size();
        c.off.assign(c.nr + 1, 0);
        c.slot.assign(c.nr, 0);
        for (size_t i = 0; i < c.nr; i++) {
            const bamrec::View &v = c.views[i];
            if (v.bad) return fail("corrupt BAM record");
            if (v.cg) b->n_cg++;
            c.off[i + 1] = c.off[i] + (v.ok ? v.n : 0);
            c.slot[i] = v.ok ? k++ : (size_t)-1;
        }
        b->n_records += (int64_t)c.nr;
        if (!b->pos.resize(k) || !b->endpos.resize(k) || !b->clip.resize(k) || !tid_of.resize(k) || !b->cig_off.resize(k) ||
            !b->cigar.resize(narena + c.off[c.nr]))
            return fail("out of host memory");
        if ((want & WANT_SEQ) && !ins.size(c, rd.threads)) return fail("out of host memory");
        if (want & WANT_SA) sa.size(c);
        return true;
    }

    // Pass 2 (parallel): the kept records copied into the columnar arrays, the products extracted.
    void copy(const Chunk &c) {
        parallel_for(rd.threads, c.nr, [&](size_t i0, size_t i1) {
            for (size_t i = i0; i < i1; i++) {
                const bamrec::View &v = c.views[i];
                if (!v.ok) continue;
                const size_t k = c.slot[i];
                if (want & WANT_SA) sa.extract(c, i);
                if (v.n) memcpy(b->cigar.data() + narena + c.off[i], v.cig, 4ull * v.n);
                b->pos[k] = v.pos;
                b->endpos[k] = bamrec::endpos(v);   // htslib bam_endpos
                b->clip[k] = (uint8_t)v.clip;
                b->cig_off[k] = narena + c.off[i];
                tid_of[k] = v.tid;
                if (want & WANT_SEQ) ins.extract(c, i);
            }
        });
    }

    void commit(const Chunk &c) {
        if (want & WANT_SA) sa.collect(c);
        narena += c.off[c.nr];
        at = c.end;
    }

    // The records, chunk by chunk; then the stage times (t_start: when the read began).
    bool records(double t_start) {
        Chunk c;
        while (!done) {
            if (buf.size() - at < 4 && !need(4)) break;   // clean EOF
            if (!scan(c)) return false;
            if (!c.nr) continue;
            view(c);
            if (!layout(c)) return false;
            copy(c);
            commit(c);
        }
        err = rd.error("");
        if (!err.empty()) return false;
        const double st[6] = {rd.t_read, rd.t_scan, rd.t_alloc_r + rd.t_alloc, rd.t_inflate, rd.t_wait, BgzfReader::now() - t_start};
        memcpy(b->stage_s, st, sizeof st);
        return true;
    }

    // The sortedness check, the one reorder -- computed once, handed to the columns and both products -- and
    // the per-tid ranges.
    bool finish() {
        const size_t n = b->pos.size();
        if (!b->cig_off.resize(n + 1)) return fail("out of host memory");
        b->cig_off[n] = narena;
        bool sorted = true;
        for (size_t i = 1; i < n && sorted; i++)
            sorted = tid_of[i] > tid_of[i - 1] || (tid_of[i] == tid_of[i - 1] && b->pos[i] >= b->pos[i - 1]);
        std::vector<size_t> idx;   // the final order of the reads; empty: the file's own
        if (!sorted) {
            idx.resize(n);
            std::iota(idx.begin(), idx.end(), 0);
            std::stable_sort(idx.begin(), idx.end(), [&](size_t x, size_t y) {
                return tid_of[x] != tid_of[y] ? tid_of[x] < tid_of[y] : b->pos[x] < b->pos[y];
            });
        }
        if (!sorted && !(permute_rows(b->cig_off, b->cigar, idx) && permute(b->pos, idx) && permute(b->endpos, idx) &&
                         permute(b->clip, idx)))
            return fail("out of host memory");
        b->tid_off.assign((size_t)n_ref + 1, 0);   // (a count per tid: the order of tid_of does not matter)
        for (size_t k = 0; k < n; k++) b->tid_off[(size_t)tid_of[k] + 1]++;
        for (int32_t t = 0; t < n_ref; t++) b->tid_off[(size_t)t + 1] += b->tid_off[(size_t)t];
        if ((want & WANT_SEQ) && !ins.finish(idx)) return fail("out of host memory");
        if (want & WANT_SA) sa.finish(idx);
        return true;
    }
};

svth_bam *bam_read_impl(const char *path, int threads, int32_t tid0, int64_t beg0, int32_t tid1, int64_t end1,
                        const svth_inflater *inf, int want, char *err, size_t errcap) {
    const double t_start = BgzfReader::now();
    Ingest in(path, threads, inf && inf->inflate ? inf : nullptr, want, tid0 >= 0, tid1, end1);
    std::string m;
    if (!in.rd.f) m = std::string("cannot open BAM: ") + path;
    else if (in.header() && in.seek_region(path, tid0, beg0) && in.records(t_start) && in.finish()) return in.b.release();
    else m = in.rd.error(in.err);
    if (err && errcap) snprintf(err, errcap, "%s", m.c_str());
    return nullptr;
}

}  // namespace

extern "C" {

svth_bam *svth_bam_read(const char *path, int threads, char *err, size_t errcap) {
    return svth_bam_read_region(path, threads, -1, 0, -1, 0, err, errcap);
}

svth_bam *svth_bam_read_region(const char *path, int threads, int32_t tid0, int64_t beg0, int32_t tid1, int64_t end1,
                               char *err, size_t errcap) {
    return svth_bam_read_ex(path, threads, tid0, beg0, tid1, end1, nullptr, err, errcap);
}

svth_bam *svth_bam_read_ex(const char *path, int threads, int32_t tid0, int64_t beg0, int32_t tid1, int64_t end1,
                           const svth_inflater *inf, char *err, size_t errcap) {
    return bam_read_impl(path, threads, tid0, beg0, tid1, end1, inf, 0, err, errcap);
}

svth_bam *svth_bam_read_seq(const char *path, int threads, int32_t tid0, int64_t beg0, int32_t tid1, int64_t end1,
                            const svth_inflater *inf, char *err, size_t errcap) {
    return bam_read_impl(path, threads, tid0, beg0, tid1, end1, inf, WANT_SEQ, err, errcap);
}

svth_bam *svth_bam_read_sa(const char *path, int threads, int32_t tid0, int64_t beg0, int32_t tid1, int64_t end1,
                           const svth_inflater *inf, char *err, size_t errcap) {
    return bam_read_impl(path, threads, tid0, beg0, tid1, end1, inf, WANT_SA, err, errcap);
}

int svth_bam_junctions(const svth_bam *b, svt_junction_view *out) {
    if (!b || !out || !b->has_sa) return 0;
    out->n = b->sa_read.size();
    out->read = b->sa_read.data();
    out->off = b->sa_off.data();
    out->seg = b->sa_seg.data();
    return 1;
}

int64_t svth_bam_n_sa_malformed(const svth_bam *b) { return b ? b->n_sa_malformed : 0; }

int svth_bam_insseq(const svth_bam *b, svt_insseq_view *out) {
    if (!b || !out || !b->has_seq) return 0;
    out->n_ins = b->ins_off.size() - 1;
    out->off = b->ins_off.data();
    out->bases = b->ins_bases.data();
    return 1;
}

int svth_bam_read_device(const char *path, int threads, const svth_dev_sink *sink, int32_t *n_targets, double *stage4,
                         char *err, size_t errcap) {
    auto fail = [&](const std::string &m) {
        if (err && errcap) snprintf(err, errcap, "%s", m.c_str());
        return 1;
    };
    if (!sink || !sink->begin || !sink->feed) return fail("no device sink");
    const double t_start = BgzfReader::now();
    // batches of whole BGZF blocks through read_next (its input buffers from the sink's allocator)
    const svth_inflater cfg{nullptr, sink->alloc, sink->release, sink->user, sink->batch_bytes};
    BgzfReader rd(path, threads, &cfg);
    if (!rd.f) return fail(std::string("cannot open BAM: ") + path);
    auto bail = [&](const std::string &m) { return fail(rd.error(m)); };
    BgzfReader::Comp c = rd.read_next();
    if (!c.ok) return bail(c.err);
    if (c.blks.empty()) return bail("not a BAM file (no BGZF blocks)");
    // the header (magic, text, references) on the host: inflate the first blocks until it is complete
    std::vector<uint8_t> h;
    size_t bi = 0, at = 0;
    ZlibRaw z;
    auto take = [&](size_t k) -> const uint8_t * {
        while (h.size() < at + k) {
            if (bi >= c.blks.size()) return nullptr;
            const svt_bgzf_block &b = c.blks[bi++];
            const size_t o = h.size();
            h.resize(o + b.ulen);
            if (!z.block(rd.cins[c.i].p + b.coff, b.clen, h.data() + o, b.ulen)) return nullptr;
        }
        at += k;
        return h.data() + at - k;
    };
    int32_t n_ref = 0;
    const std::string he = parse_header(take, " (or longer than one batch)", n_ref, nullptr);
    if (!he.empty()) return bail(he);
    if (n_targets) *n_targets = n_ref;
    char e[512] = {0};
    if (sink->begin(sink->user, n_ref, e, sizeof e) != 0) return bail(e[0] ? e : "device sink: begin failed");
    // the batches: the next one read and scanned by a helper thread while this one is decoded
    double t_feed = 0, t_wait = 0;
    uint64_t skip = at;
    for (;;) {
        if (!rd.eof || rd.carry_n) rd.pending_comp = std::async(std::launch::async, [&rd] { return rd.read_next(); });
        const double t0 = BgzfReader::now();
        const int rc = sink->feed(sink->user, rd.cins[c.i].p, c.p, c.blks.data(), c.blks.size(), skip, e, sizeof e);
        t_feed += BgzfReader::now() - t0;
        skip = 0;
        if (rc != 0) return bail(e[0] ? e : "device sink: feed failed");
        if (!rd.pending_comp.valid()) break;
        const double t1 = BgzfReader::now();
        c = rd.pending_comp.get();
        t_wait += BgzfReader::now() - t1;
        if (!c.ok) return bail(c.err);
        if (c.blks.empty()) break;
    }
    if (stage4) {   // (no batch is pending here: the helper thread has finished)
        stage4[0] = rd.t_read;
        stage4[1] = t_feed;
        stage4[2] = t_wait + rd.t_alloc_r;
        stage4[3] = BgzfReader::now() - t_start;
    }
    return 0;
}

void svth_bam_free(svth_bam *b) { delete b; }

void svth_bam_view(const svth_bam *b, svt_pileup_view *v) {
    v->n_targets = (int32_t)b->names.size();
    v->tid_off = b->tid_off.data();
    v->pos = b->pos.data();
    v->endpos = b->endpos.data();
    v->cig_off = b->cig_off.data();
    v->cigar = b->cigar.data();
    v->clip = b->clip.data();
}

int32_t svth_bam_n_targets(const svth_bam *b) { return (int32_t)b->names.size(); }
const char *svth_bam_target_name(const svth_bam *b, int32_t t) {
    return (t >= 0 && (size_t)t < b->names.size()) ? b->names[(size_t)t].c_str() : nullptr;
}
int64_t svth_bam_n_records(const svth_bam *b) { return b->n_records; }
int64_t svth_bam_n_cg_restored(const svth_bam *b) { return b->n_cg; }
void svth_bam_stage_seconds(const svth_bam *b, double *s6) { memcpy(s6, b->stage_s, sizeof b->stage_s); }

}  // extern "C"
