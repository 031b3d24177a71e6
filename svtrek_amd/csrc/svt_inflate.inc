// svt_inflate.inc -- BGZF inflate on the device: one wave per block (included by svt_engine.hip).
//
// What the reference gets from htslib's bgzf_read (refinement.c:117 sam_itr_next -> bam_read1 ->
// bgzf_read -> zlib inflate) is each BGZF block's bytes; this decodes the same raw DEFLATE
// stream (RFC 1951) and accepts / rejects streams as zlib's inflate does (inftrees.c's rules for
// over-subscribed and incomplete codes, inflate.c's distance / length / ISIZE checks).
//
// DEFLATE is one serial bitstream per block, so a block's symbols are decoded by its wave as
// wave-uniform work: the bit buffer, the table lookups' results and the output position are kept
// by every lane alike (vector registers: the per-symbol arithmetic runs on the vector units; the
// scalar unit only takes the data-dependent branches, iw_codes), and the vector units also do the
// wide parts --
//   * building each code's tables: 64 symbols (counts, canonical order) or 64 root-table entries
//     a step, ballots instead of serial loops;
//   * (the compressed stream is read one dword ahead: vector loads in the codes loop, scalar loads
//     in the headers);
//   * output: every byte goes to an LDS ring of the last 2 KiB, stored 256 bytes (a dword a lane)
//     at a time; a match copies 64 bytes a step from the ring, or from the stored output when its
//     distance is longer (byte i of a match of distance d is byte (i mod d) of the d bytes before
//     it, so every source byte precedes the match).
// Tables: a 9-bit root table for literal/length codes, 8 bits for distances (iw_lent's entry
// formats), longer codes by the canonical per-length walk.  4992 B of LDS a wave, so a CU holds
// 32 waves (8 a SIMD): the latency of each wave's serial chain (LDS lookups, the loads of a far
// match) is hidden by the other waves' work, and a batch of >= 8192 blocks fills the chip.

constexpr int INF_OK = 0, INF_EDATA = 1, INF_EOUT = 2, INF_EIN = 3;
constexpr int INF_FIXED = 0, INF_CODES = 1, INF_LENS = 2;   // zlib inflate_table's code kinds
#ifndef SVT_IW_LB
#define SVT_IW_LB 9
#endif
constexpr int IW_LB = SVT_IW_LB, IW_DB = 8, IW_CB = 7;       // root table bits: lit/len, dist, code lengths
constexpr uint32_t IW_LIT = 0x8000u;                          // (u16 entries) root entry flag: a literal
// Literal/length root entries (u16; 0 = a code longer than the root table):
//   literal:      byte | code length << 9 | IW_LIT                       (>= 0x8000)
//   length code:  (base length - 3) | extra bits << 8 | code length << 11 (0x800 .. 0x7fff;
//                 RFC 1951 3.2.5)
//   end of block: IW_EOB | code length;  symbols 286, 287: IW_BAD | code length  (< 0x800)
// so a match's length is one add and one bit-field extract (no per-symbol table arithmetic), and
// everything that leaves the fast path -- the end of the block, a bad symbol, a code longer than
// the root table (entry 0) -- is one compare: entry < IW_FAST.
// Distance and code-length-code entries: symbol | code length << 9.
constexpr uint32_t IW_EOB = 0x100u, IW_BAD = 0x200u, IW_FAST = 0x800u;
#ifndef SVT_IW_RING
#define SVT_IW_RING 2048
#endif
// iw_vgpr: a copy the compiler must keep per lane (the vector-side decode state, iw_codes).
__device__ __forceinline__ uint32_t iw_vgpr(uint32_t x) {
    asm("" : "+v"(x));
    return x;
}

struct IwCode {             // a code's canonical form, per length 1..15
    uint16_t cnt[16], offs[16], first[16];
};
struct IwLds {
    uint16_t lit[1 << IW_LB];   // root entries (iw_lent's format; 0 = longer code)
    uint16_t dst[1 << IW_DB];
    union {
        uint16_t cl[1 << IW_CB];    // the code-length code of a dynamic block's header
        uint32_t stage[WAVE];       // (while a block's codes are decoded) a far match's source (iw_codes)
    };
    uint16_t lsym[288];         // symbols in canonical order (by length, then symbol)
    uint16_t dsym[32];
    IwCode lc, dc;
    uint8_t len[320];           // code lengths: literal/length 0..287, distance from 288
    uint8_t ring[SVT_IW_RING];  // the last IW_RING output bytes (IwOut)
};

__device__ __forceinline__ uint32_t iw_rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// Wave-local ordering of LDS and global memory: the wave's own stores (any lane) are complete and
// visible to its later loads (any lane).  One wave per workgroup, so this is the workgroup barrier.
__device__ __forceinline__ void iw_sync() { __syncthreads(); }
// Closes a lane-divergent region (stores by some lanes): a block of its own where the lanes
// reconverge, so that the compiler does not merge that join with joins of the scalar state's
// branches -- which would make the scalar state per-lane (VGPRs, divergent branches).
__device__ __forceinline__ void iw_join() { __builtin_amdgcn_wave_barrier(); }

// RFC 1951 3.2.5 length / distance bases and extra bits (arithmetic forms of the RFC's tables)
__device__ __forceinline__ uint32_t iw_lext(uint32_t i) { return i < 8 || i == 28 ? 0u : (i - 4) >> 2; }
__device__ __forceinline__ uint32_t iw_lbase(uint32_t i) {
    return i < 8 ? 3u + i : i == 28 ? 258u : ((4u + (i & 3)) << iw_lext(i)) + 3u;
}
// a literal/length symbol's root entry for a code of length cl (format above)
__device__ __forceinline__ uint32_t iw_lent(uint32_t sy, uint32_t cl) {
    if (sy < 256u) return sy | cl << 9 | IW_LIT;
    if (sy == 256u) return IW_EOB | cl;
    if (sy > 285u) return IW_BAD | cl;
    return (iw_lbase(sy - 257u) - 3u) | iw_lext(sy - 257u) << 8 | cl << 11;
}
__device__ __forceinline__ uint32_t iw_dext(uint32_t i) { return i < 4 ? 0u : (i - 2) >> 1; }
__device__ __forceinline__ uint32_t iw_dbase(uint32_t i) { return i < 4 ? 1u + i : ((2u + (i & 1)) << iw_dext(i)) + 1u; }
// the code-length code's transmission order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
__device__ __forceinline__ uint32_t iw_ord(uint32_t i) {
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 |
                        10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
}

// The bit reader of the block headers (iw_codes keeps its own copy of the state in vector
// registers).  The block's data starts `skip` (< 4) bytes into the dword at `src`; dwords from the
// one holding the last data byte on read as zero.  The stream is read with scalar loads
// (wave-uniform addresses, through the scalar cache), one dword ahead of its use.  fill() keeps
// >= 32 bits buffered, enough for any one step (a code of <= 15 bits + <= 13 extra bits) after it.
typedef const uint32_t __attribute__((address_space(4))) *iw_cptr;   // constant space: scalar loads
struct IwBits {
    iw_cptr src;
    uint32_t nd;        // dwords holding data
    uint32_t dw;        // dwords taken into bb so far
    uint32_t pre;       // dword dw (0 past the data)
    uint32_t skip, clen;
    uint64_t bb;
    uint32_t nb;

    __device__ __forceinline__ uint32_t ld(uint32_t i) const { return i < nd ? src[i] : 0u; }
    __device__ __forceinline__ void init(const uint32_t *s, uint32_t skip_, uint32_t clen_) {
        src = (iw_cptr)s;
        skip = skip_;
        clen = clen_;
        nd = (skip_ + clen_ + 3u) >> 2;
        dw = 0;
        pre = ld(0);
        bb = 0;
        nb = 0;
        fill();
        drop(8 * skip_);
    }
    __device__ __forceinline__ void fill() {
        if (nb < 32) {
            bb |= (uint64_t)pre << nb;
            nb += 32;
            pre = ld(++dw);
        }
    }
    __device__ __forceinline__ uint32_t peek(uint32_t k) const { return (uint32_t)bb & ((1u << k) - 1u); }
    __device__ __forceinline__ void drop(uint32_t k) {
        bb >>= k;
        nb -= k;
    }
    __device__ __forceinline__ uint32_t get(uint32_t k) {
        const uint32_t v = peek(k);
        drop(k);
        return v;
    }
    __device__ __forceinline__ bool past() const {   // consumed more than clen bytes
        return 32ull * dw - nb - 8ull * skip > 8ull * clen;
    }
};

// Output.  Positions count from the block's dword-aligned base `ob`; the block owns [a0, aend)
// (a0 < 4).  Every byte (literal or match) is first written to an LDS ring holding the last
// IW_RING positions; each completed 256-byte chunk is stored with one dword store a lane.  A
// match copies from the ring when its distance fits (dist <= IW_RING), otherwise from the stored
// output (its source then lies >= IW_RING - 258 positions back, in chunks stored long before).
// Chunk 0 (bytes below a0 belong to the previous block) and the block's last chunk are stored
// byte-exactly.
constexpr uint32_t IW_RING = SVT_IW_RING, IW_RMASK = IW_RING - 1;
// A match's copy writes the 64 ring positions from the output position on (its bytes, then
// don't-care bytes that the output overwrites before any read): the ring positions IW_AHEAD
// below a wrap are stale, so a match reads the ring only up to IW_RING - IW_AHEAD back (a
// longer distance reads the stored output, in chunks stored long before).
constexpr uint32_t IW_AHEAD = 64u;
static_assert((IW_RING & IW_RMASK) == 0 && IW_RING >= 1024, "ring: a power of two >= 1 KiB");
struct IwOut {
    uint8_t *ob;
    uint8_t *ring;
    uint32_t a, a0, aend, fl;   // next position, block start / end, first position not stored

    __device__ __forceinline__ void init(uint8_t *base, uint8_t *lds_ring, uint32_t a0_, uint32_t ulen) {
        ob = base;
        ring = lds_ring;
        a = a0 = a0_;
        aend = a0_ + ulen;
        fl = 0;
    }
    // store the bytes [lo, hi) of the chunk at fl (one dword a lane; byte-exact at the ends)
    __device__ __forceinline__ void store_part(uint32_t w, uint32_t lo, uint32_t hi) {
        const uint32_t wa = fl + 4u * threadIdx.x;
        if (wa >= lo && wa + 4u <= hi) {
            *reinterpret_cast<uint32_t *>(ob + wa) = w;
        } else if (wa < hi && wa + 4u > lo) {
#pragma unroll
            for (uint32_t j = 0; j < 4; j++)
                if (wa + j >= lo && wa + j < hi) ob[wa + j] = (uint8_t)(w >> (8 * j));
        }
        iw_join();
    }
    __device__ __forceinline__ uint32_t chunk_word() const {
        return *reinterpret_cast<const uint32_t *>(ring + ((fl + 4u * threadIdx.x) & IW_RMASK));
    }
    __device__ __forceinline__ void store_chunk() {   // [fl, fl + 256), complete
        const uint32_t w = chunk_word();
        if (fl != 0 || a0 == 0)
            *reinterpret_cast<uint32_t *>(ob + fl + 4u * threadIdx.x) = w;
        else
            store_part(w, a0, 256u);
        fl += 256u;
    }
    __device__ __forceinline__ void finish() {   // [fl, aend)
        if (aend > fl) store_part(chunk_word(), fl > a0 ? fl : a0, aend);
    }
    // a literal: every lane writes the same byte (no exec-mask round trip per byte); the block's
    // end is checked when a chunk completes (false: the literals ran past it), so a run of
    // literals pays no per-byte bound check and never stores past the block
    __device__ __forceinline__ bool lit(uint32_t s) {
        ring[a & IW_RMASK] = (uint8_t)s;
        iw_join();
        if ((++a & 255u) == 0) {
            if (a > aend) return false;
            store_chunk();
        }
        return true;
    }
};

// Build a code's tables from n lengths (L.len-style bytes at `len`): the root table of ROOT bits
// and the canonical form.  False for a code zlib's inflate_table rejects: over-subscribed, or
// incomplete where that is not allowed (INF_CODES never, INF_LENS only for a single code of
// length 1; a code with no symbols builds a table on which every lookup fails, as zlib's does).
//
// Per-length quantities live one per lane (lane l: length l's count, canonical offset and first
// code), read out with v_readlane where a step needs one: the build then holds few scalar
// registers, and the decoder's scalar state stays in registers around it.
template <int ROOT, int NMAX, typename T, bool LITLEN = false>
__device__ __forceinline__ bool iw_build(const uint8_t *len, uint32_t n, T *tab, uint16_t *sym, IwCode &cd,
                                         int kind) {
    constexpr int NJ = (NMAX + 63) / 64;
    constexpr int NE = (1 << ROOT) / 64;   // root entries a lane
    const uint32_t ln = threadIdx.x;
    const uint64_t below = (1ull << ln) - 1ull;
    uint32_t v[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) v[j] = 64u * j + ln < n ? len[64u * j + ln] : 0u;
    uint32_t cnt = 0;   // lane l: codes of length l
#pragma unroll 1
    for (int l = 1; l < 16; l++) {
        uint32_t c = 0;
#pragma unroll
        for (int j = 0; j < NJ; j++) c += (uint32_t)__popcll(__ballot(v[j] == (uint32_t)l));
        cnt = ln == (uint32_t)l ? c : cnt;
    }
    int left = 1, mx = 0;
    uint32_t off = 0, first = 0, ro = 0, rf = 0;   // lane l: offset, first code; running sums
#pragma unroll 1
    for (int l = 1; l < 16; l++) {
        const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)cnt, l);
        left = 2 * left - (int)c;
        if (c) mx = l;
        off = ln == (uint32_t)l ? ro : off;
        first = ln == (uint32_t)l ? rf : first;
        ro += c;
        rf = (rf + c) << 1;
        if (left < 0) return false;   // over-subscribed
    }
    if (kind != INF_FIXED && mx > 0 && left > 0 && (kind == INF_CODES || mx != 1)) return false;   // incomplete
    // canonical order: symbol s of length l goes to offset l + (symbols of length l before s)
    uint32_t run = 0;
#pragma unroll
    for (int j = 0; j < NJ; j++) {
#pragma unroll 1
        for (int l = 1; l < 16; l++) {
            const uint64_t m = __ballot(v[j] == (uint32_t)l);
            const uint32_t at = (uint32_t)__builtin_amdgcn_readlane((int)(off + run), l);
            if (v[j] == (uint32_t)l) sym[at + (uint32_t)__popcll(m & below)] = (uint16_t)(64u * j + ln);
            iw_join();
            run += ln == (uint32_t)l ? (uint32_t)__popcll(m) : 0u;
        }
    }
    if (ln < 16) {
        cd.cnt[ln] = (uint16_t)cnt;
        cd.offs[ln] = (uint16_t)off;
        cd.first[ln] = (uint16_t)first;
    }
    iw_sync();
    // root entries, NE a lane: entry e holds the code whose bits (stream order) prefix e.  (Loops
    // over lanes' items keep wave-uniform trip counts: a loop exit that differs by lane would make
    // every value live across it -- the decoder's scalar state -- per-lane to the compiler.)
    uint32_t code[NE], ent[NE];
#pragma unroll
    for (int t = 0; t < NE; t++) {
        code[t] = __brev(64u * t + ln) >> (32 - ROOT);   // the ROOT bits, first bit MSB
        ent[t] = 0;
    }
#pragma unroll 1
    for (int l = 1; l <= ROOT; l++) {
        const uint32_t f = (uint32_t)__builtin_amdgcn_readlane((int)first, l);
        const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)cnt, l);
        const uint32_t o = (uint32_t)__builtin_amdgcn_readlane((int)off, l);
#pragma unroll
        for (int t = 0; t < NE; t++) {
            const uint32_t p = (code[t] >> (ROOT - l)) - f;
            ent[t] = ent[t] == 0 && p < c ? (o + p) | (uint32_t)l << 9 : ent[t];
        }
    }
#pragma unroll
    for (int t = 0; t < NE; t++) {
        const uint32_t sy = sym[ent[t] & 511u];
        tab[64u * t + ln] = !ent[t] ? (T)0 : LITLEN ? (T)iw_lent(sy, ent[t] >> 9) : (T)(sy | (ent[t] & ~511u));
    }
    iw_sync();
    return true;
}

// A code longer than the root table (after its root entry read 0): the canonical walk over the
// lengths past ROOT.  0xffff: no code of this stream matches.
template <int ROOT>
__device__ __forceinline__ uint32_t iw_slow(IwBits &br, const uint16_t *sym, const IwCode &cd) {
    const uint32_t code = __brev((uint32_t)br.bb) >> 17;   // the next 15 bits, first bit MSB
    for (uint32_t l = ROOT + 1; l < 16; l++) {
        const uint32_t p = (code >> (15 - l)) - iw_rfl(cd.first[l]);
        if (p < iw_rfl(cd.cnt[l])) {
            br.drop(l);
            return iw_rfl(sym[iw_rfl(cd.offs[l]) + p]);
        }
    }
    return 0xffffu;
}

// One symbol (after fill()).
template <int ROOT>
__device__ __forceinline__ uint32_t iw_sym(IwBits &br, const uint16_t *tab, const uint16_t *sym, const IwCode &cd) {
    const uint32_t e = iw_rfl(tab[br.peek(ROOT)]);
    if (e) {
        br.drop((e >> 9) & 15u);
        return e & 511u;
    }
    return iw_slow<ROOT>(br, sym, cd);
}

// A dynamic block's header (RFC 1951 3.2.7): the code-length code, then the literal/length and
// distance code lengths (a repeat may run from one list into the other) into L.len.
__device__ __forceinline__ int iw_dynamic(IwLds &L, IwBits &br, uint32_t &ndist_out) {
    const uint32_t ln = threadIdx.x;
    br.fill();
    const uint32_t nlen = br.get(5) + 257, ndist = br.get(5) + 1, ncode = br.get(4) + 4;
    if (nlen > 286 || ndist > 30) return INF_EDATA;
    uint32_t mine = 0;
    for (uint32_t i = 0; i < ncode; i++) {
        br.fill();
        const uint32_t x = br.get(3);
        if (ln == iw_ord(i)) mine = x;
    }
    if (ln < 19) L.len[ln] = (uint8_t)mine;
    iw_sync();
    if (!iw_build<IW_CB, 19>(L.len, 19, L.cl, L.lsym, L.lc, INF_CODES)) return INF_EDATA;
    const uint32_t tot = nlen + ndist;
    uint32_t i = 0, prev = 0;
    while (i < tot) {
        br.fill();
        const uint32_t s = iw_sym<IW_CB>(br, L.cl, L.lsym, L.lc);
        uint32_t val, rep;
        if (s < 16) {
            val = s;
            rep = 1;
        } else if (s == 16) {
            if (i == 0) return INF_EDATA;
            val = prev;
            rep = 3 + br.get(2);
        } else if (s == 17) {
            val = 0;
            rep = 3 + br.get(3);
        } else if (s == 18) {
            val = 0;
            rep = 11 + br.get(7);
        } else {
            return INF_EDATA;
        }
        if (i + rep > tot) return INF_EDATA;
        for (uint32_t j0 = 0; j0 < rep; j0 += 64u) {
            const uint32_t j = i + j0 + ln;
            if (j0 + ln < rep) L.len[j < nlen ? j : 288 + j - nlen] = (uint8_t)val;
        }
        iw_join();
        i += rep;
        prev = val;
    }
    for (uint32_t j0 = nlen; j0 < 288; j0 += 64u)
        if (j0 + ln < 288) L.len[j0 + ln] = 0;
    iw_sync();
    if (iw_rfl(L.len[256]) == 0) return INF_EDATA;   // no end-of-block code
    ndist_out = ndist;
    return INF_OK;
}

__device__ __forceinline__ void iw_fixed(IwLds &L) {   // RFC 1951 3.2.6 (its 30 distance codes of 5 bits)
    const uint32_t ln = threadIdx.x;
    for (uint32_t s0 = 0; s0 < 318; s0 += 64u) {
        const uint32_t s = s0 + ln;
        if (s < 318) L.len[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
    }
    iw_sync();
}

// SVT_PHASE_PROF (diagnostic builds): lane 0 adds per-block counts and times to ph_prof
// (svt_diag_phase): [0] header + table ticks, [1] code ticks, [2] deflate blocks, [3] dynamic
// ones, [4] stored bytes, [5] literals, [6] matches, [7] match bytes, [8] far matches, [9] BGZF
// blocks, [10] BGZF block ticks.
#if SVT_PHASE_PROF
#define IWP(...) __VA_ARGS__
#define IWP_ADD(i, v) \
    if (threadIdx.x == 0) PH_ADD(i, v)
#else
#define IWP(...)
#define IWP_ADD(i, v)
#endif

// Literals and matches until the end-of-block code.  The decoder's per-symbol state -- the 64-bit
// bit buffer, its fill and the output position -- lives in vector registers (every lane the same
// value), and so does all per-symbol arithmetic: a match's length and distance bases and extra
// bits, its bound checks, its copy.  Only the data-dependent branches (literal or not, a refill, a
// code longer than the root table, a chunk completed) reach the scalar unit, as one
// readfirstlane and a compare each.  The decode is one serial chain per block and a CU has one
// scalar unit: with the state on the scalar side the kernel was bound by it (34 SALU instructions
// per output byte, r04_infpmc; ~100 per match, r05_O), while the vector units issue two wave-wide
// instructions a cycle and were mostly idle.
__device__ __forceinline__ int iw_codes(IwLds &L, IwBits &br, IwOut &o) {
    IWP(uint32_t nlit = 0; uint32_t nmat = 0; uint32_t nmb = 0; uint32_t nfar = 0;)
    IWP(struct Flush { uint32_t &a, &b, &c, &d; __device__ ~Flush() { IWP_ADD(5, a); IWP_ADD(6, b); IWP_ADD(7, c); IWP_ADD(8, d); } } flush_{nlit, nmat, nmb, nfar};)
    const uint32_t k = threadIdx.x;
    uint32_t bl = iw_vgpr((uint32_t)br.bb), bh = iw_vgpr((uint32_t)(br.bb >> 32));
    uint32_t vnb = iw_vgpr(br.nb), va = iw_vgpr(o.a);
    int rc = INF_OK;
    constexpr uint32_t M = (1u << IW_LB) - 1u, MD = (1u << IW_DB) - 1u;
    auto vdrop = [&](uint32_t n) {
        const uint64_t x = ((uint64_t)bh << 32 | bl) >> n;
        bl = (uint32_t)x;
        bh = (uint32_t)(x >> 32);
        vnb -= n;
    };
    // The bitstream is prefetched one dword ahead with a VECTOR load (vpre, every lane the same
    // word): a scalar load would share the LDS lookups' wait counter, so the next table lookup
    // after every refill would wait for it too; the vector load's counter is waited on only by
    // the refill that consumes it.  (Loads stay inside the block's dwords; past them: 0.)
    const __attribute__((address_space(1))) uint32_t *gs =
        (const __attribute__((address_space(1))) uint32_t *)(br.src);
    const uint32_t ndl = br.nd > 0u ? br.nd - 1u : 0u;
    uint32_t vdw = iw_vgpr(br.dw), vpre = iw_vgpr(br.pre);
    auto vfill = [&]() {   // br.fill(): >= 32 bits buffered
        if (iw_rfl(vnb) < 32u) {   // vpre: dword vdw as loaded (zero past the block's dwords here)
            const uint64_t x = ((uint64_t)bh << 32 | bl) | ((uint64_t)(vdw < br.nd ? vpre : 0u) << vnb);
            bl = (uint32_t)x;
            bh = (uint32_t)(x >> 32);
            vnb += 32u;
            vdw += 1u;
            vpre = gs[min(vdw, ndl)];
        }
    };
    auto tosc = [&]() {   // the reader's state to the scalar reader (a long code's canonical walk)
        br.bb = (uint64_t)iw_rfl(bh) << 32 | iw_rfl(bl);
        br.nb = iw_rfl(vnb);
        br.dw = iw_rfl(vdw);
        br.pre = iw_rfl(vdw < br.nd ? vpre : 0u);
    };
    auto tovec = [&]() {
        bl = iw_vgpr((uint32_t)br.bb);
        bh = iw_vgpr((uint32_t)(br.bb >> 32));
        vnb = iw_vgpr(br.nb);
        vdw = iw_vgpr(br.dw);
        vpre = iw_vgpr(br.pre);
    };
    // A far match (source past the ring: the stored output) is copied by an LDS-DMA load of the 256
    // bytes from its source's dword on into L.stage, left in flight: its bytes go to the ring only
    // when something needs them -- a match reading them, the store of the chunk holding them, the
    // next far match, the end of the block's codes -- so the load's round trip overlaps the
    // decode of the symbols after it (the far loads cost 11 % of the kernel when waited on at once,
    // r05_X).  A DMA load, not a load into a register: the compiler copies registers at control-flow
    // joins, and a copy of a loaded register waits for the load.  Later output is written past the
    // pending bytes, and their ring slots are not reused before their chunk is stored.
    bool pend = false;
    uint32_t pdst = 0, plen = 0, pofs = 0;
    auto flush = [&]() {
        if (pend) {
            __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0): the staged bytes have landed
            const uint8_t *sb = reinterpret_cast<const uint8_t *>(L.stage) + pofs;
            if (k < plen) o.ring[(pdst + k) & IW_RMASK] = sb[k];
            iw_join();
            pend = false;
        }
    };
    // One symbol an iteration -- a literal or a match -- with one uniform branch between the two
    // and one compare for everything that leaves the fast path (entry < IW_FAST): no inner loops
    // and no flag-carried breaks, which cost the decode more scalar instructions than its work.
    for (;;) {
        vfill();   // >= 32 bits: a root code (<= IW_LB bits, else iw_slow's <= 15) and a length's extra bits (<= 5)
        uint32_t ev = L.lit[bl & M], e = iw_rfl(ev);
        if (e < IW_FAST) {   // the end of the block, a bad symbol, or a longer code
            if (e & IW_EOB) { vdrop(e & 15u); break; }
            if (e) { rc = INF_EDATA; break; }
            tosc();
            const uint32_t su = iw_slow<IW_LB>(br, L.lsym, L.lc);
            tovec();
            if (su == 256u) break;
            if (su > 285u) { rc = INF_EDATA; break; }   // (0xffff: no code)
            ev = iw_vgpr(iw_lent(su, 0u));               // (its bits are dropped)
            e = su < 256u ? IW_LIT : IW_FAST;
        }
        if (e & IW_LIT) {   // a literal
            vdrop((ev >> 9) & 15u);
            o.ring[va & IW_RMASK] = (uint8_t)ev;
            iw_join();
            va += 1u;
            IWP(nlit += 1;)
        } else {   // a match: length (RFC 1951 3.2.5), distance, checks, copy -- on the lane copies
            vdrop((ev >> 11) & 15u);
            const uint32_t lx = (ev >> 8) & 7u;
            const uint32_t len = (ev & 255u) + 3u + __builtin_amdgcn_ubfe(bl, 0, lx);
            vdrop(lx);
            vfill();   // >= 32 bits: a distance code (<= 15) and its extra bits (<= 13)
            const uint32_t dv = L.dst[bl & MD];
            uint32_t dsym;
            if (iw_rfl(dv)) {
                dsym = dv & 511u;
                vdrop((dv >> 9) & 15u);
            } else {
                tosc();
                dsym = iw_vgpr(iw_slow<IW_DB>(br, L.dsym, L.dc));   // 0xffff: no code (>= 30 below)
                tovec();
            }
            const uint32_t dx = iw_dext(dsym) & 31u;   // (dsym >= 30: an error below)
            const uint32_t dist = iw_dbase(dsym) + __builtin_amdgcn_ubfe(bl, 0, dx);
            vdrop(dx);
            const uint32_t err =
                dsym >= 30u || dist > va - o.a0 ? (uint32_t)INF_EDATA : va + len > o.aend ? (uint32_t)INF_EOUT : 0u;
            if (const uint32_t eu = iw_rfl(err)) { rc = (int)eu; break; }
            const uint32_t du = iw_rfl(dist), lu = iw_rfl(len);
            IWP(nmat += 1; nmb += lu; nfar += du > IW_RING - IW_AHEAD ? 1u : 0u;)
            // byte i of the match = byte (i mod dist) after src; every lane stores (the ring's
            // positions past the match are rewritten before any read: IW_AHEAD), lanes past the
            // match read bytes before va (the ring's, or stored chunks: a far source ends
            // >= IW_RING - IW_AHEAD - 64 before va).  The ring and the stored output are read in
            // separate loops (as one loop the compiler reads both through one flat pointer, which
            // waits on the vector-memory counter for ring bytes).
            const uint32_t src = va - dist;
            auto at = [&](uint32_t i) -> uint32_t {
                if (du >= lu) return src + i;   // no overlap (the common case)
                return src + (i < len ? i % dist : 0u);
            };
            if (du <= IW_RING - IW_AHEAD) {
                const uint32_t su = iw_rfl(src);
                if (pend && su < pdst + plen && su + min(du, lu) > pdst) flush();   // it reads them
                const __attribute__((address_space(3))) uint8_t *rg =
                    (const __attribute__((address_space(3))) uint8_t *)(o.ring);
                for (uint32_t j = 0; j < lu; j += 64u) {
                    const uint32_t v = rg[at(j + k) & IW_RMASK];
                    o.ring[(va + j + k) & IW_RMASK] = (uint8_t)v;
                    iw_join();
                }
            } else {
                const __attribute__((address_space(1))) uint8_t *ob =
                    (const __attribute__((address_space(1))) uint8_t *)(o.ob);
                flush();   // (one staged match at a time)
                if (lu <= 64u) {   // no overlap (du > lu): the 256 bytes from src's dword, left in flight
                    const uint32_t s4 = src & ~3u;
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(ob + s4 + 4u * k),
                                                     (__attribute__((address_space(3))) void *)L.stage, 4, 0, 0);
                    pend = true;
                    pdst = iw_rfl(va);
                    plen = lu;
                    pofs = iw_rfl(src) & 3u;
                } else {
                    for (uint32_t j = 0; j < lu; j += 64u) {
                        const uint32_t v = ob[at(j + k)];
                        o.ring[(va + j + k) & IW_RMASK] = (uint8_t)v;
                        iw_join();
                    }
                }
            }
            va += len;
        }
        // completed chunks: the block's end (literals), then their stores
        const uint32_t au = iw_rfl(va);
        if (au - o.fl >= 256u) {
            if (o.fl + 256u > o.aend) { rc = INF_EOUT; break; }
            if (pend && pdst < au) flush();   // (the pending bytes lie in [fl, au))
            do o.store_chunk(); while (au - o.fl >= 256u);
        }
    }
    flush();
    iw_join();
    tosc();
    o.a = iw_rfl(va);
    return rc;
}

// Inflate one block: clen bytes of raw DEFLATE at `in` to exactly ulen bytes at `out`.
__device__ int iw_block(IwLds &L, const uint8_t *__restrict__ in, uint32_t clen, uint8_t *__restrict__ out,
                        uint32_t ulen) {
    IwBits br;
    const uint32_t skip = (uint32_t)((uintptr_t)in & 3u);
    br.init(reinterpret_cast<const uint32_t *>(in - skip), skip, clen);
    IwOut o;
    const uint32_t a0 = (uint32_t)((uintptr_t)out & 3u);
    o.init(out - a0, L.ring, a0, ulen);
    IWP(const long long tb0 = wall_clock64(); IWP_ADD(9, 1);)
    IWP(struct BFlush { long long t; __device__ ~BFlush() { IWP_ADD(10, wall_clock64() - t); } } bflush_{tb0};)
    for (;;) {
        br.fill();
        IWP(const long long th0 = wall_clock64(); IWP_ADD(2, 1);)
        const uint32_t hdr = br.get(3), type = hdr >> 1;
        if (type == 0) {   // stored
            br.drop(br.nb & 7u);
            br.fill();
            const uint32_t n = br.get(16), nn = br.get(16);
            if ((n ^ 0xffffu) != nn) return INF_EDATA;
            if (o.a + n > o.aend) return INF_EOUT;
            IWP_ADD(4, n);
            for (uint32_t i = 0; i < n; i++) {
                br.fill();
                (void)o.lit(br.get(8));   // (n fits: checked above)
            }
        } else if (type == 1 || type == 2) {
            uint32_t ndist = 30;
            if (type == 1) {
                iw_fixed(L);
            } else if (const int rc = iw_dynamic(L, br, ndist)) {
                return rc;
            }
            const int kind = type == 1 ? INF_FIXED : INF_LENS;
            if (!iw_build<IW_LB, 288, uint16_t, true>(L.len, 288, L.lit, L.lsym, L.lc, kind) ||
                !iw_build<IW_DB, 32>(L.len + 288, ndist, L.dst, L.dsym, L.dc, kind))
                return INF_EDATA;
            IWP(const long long th1 = wall_clock64(); IWP_ADD(0, th1 - th0); IWP_ADD(3, type == 2 ? 1u : 0u);)
            const int rc_ = iw_codes(L, br, o);
            IWP(IWP_ADD(1, wall_clock64() - th1);)
            if (rc_) return rc_;
        } else {
            return INF_EDATA;
        }
        if (br.past()) return INF_EIN;
        if (hdr & 1u) break;   // BFINAL
    }
    if (o.a != o.aend) return INF_EOUT;
    o.finish();
    return INF_OK;
}

// One wave (workgroup) per block; the grid strides over blocks [b0, b0 + n) of the batch.  err:
// the first bad block (its index in the batch).
// 8 waves per SIMD (<= 64 VGPRs; the 4992 B of LDS a wave let a CU hold 32): the decode is a
// serial chain per block, and more chains in flight hide more of its latency -- 29.4 GB/s against
// 25.8 at 6 waves with a 10-bit root (r05_X, r05_Y)
#ifndef SVT_INF_WAVES
#define SVT_INF_WAVES 8
#endif
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SVT_INF_WAVES, SVT_INF_WAVES))) void inflate_kernel(const uint8_t *__restrict__ comp,
                                                     const svt_bgzf_block *__restrict__ blk, uint32_t b0, uint32_t n,
                                                     uint8_t *__restrict__ out, uint32_t *__restrict__ err) {
    __shared__ IwLds L;
    for (uint32_t b = blockIdx.x; b < n; b += gridDim.x) {
        const svt_bgzf_block k = blk[b0 + b];
        const int rc = iw_block(L, comp + k.coff, k.clen, out + k.uoff, k.ulen);
        if (rc != INF_OK && threadIdx.x == 0) atomicMin(err, b0 + b);
        iw_sync();   // L is rebuilt by the next block
    }
}
constexpr unsigned INF_GRID = 1u << 20;   // workgroups at most (one block each; more stride)
