// vcf_audit.cpp -- VCF record parsing (A1) and refined-call printing (A11) for the
// `svtrek audt` drop-in.  Behaviour follows the reference byte for byte:
//   parse:  thread_func, reference audit.c:62-173 (strtok_r tokenisation, strstr
//           "SVTYPE=" / "END=" -- the latter also matching inside "CIEND=" --, strtol
//           into uint32, the length inference when SVTYPE is absent, the 50-bp filter);
//   print:  audit.c:176-232 printf formats (%u / %d of uint32 values, NA for 0xFFFFFFFF).
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <string>
#include <atomic>
#include <thread>
#include <vector>

#include "svtrek_host.h"

namespace {

constexpr int SV_MIN_LENGTH = 50;   // params.h:33

int sv_type_of(const char *s) {     // parse_sv_type, audit.c:3-11
    if (!strcmp(s, "INS") || !strcmp(s, "INS:ME")) return SVT_INS;
    if (!strcmp(s, "DEL") || !strcmp(s, "DEL:ME")) return SVT_DEL;
    if (!strcmp(s, "INV")) return SVT_INV;
    if (!strcmp(s, "DUP")) return SVT_DUP;
    if (!strcmp(s, "TRA")) return SVT_TRA;
    if (!strcmp(s, "BND")) return SVT_BND;
    return SVT_UNKNOWN;
}

// copy the value after `key` up to ';' (at most cap-1 bytes), as audit.c:119-129 / :148-158
void info_value(const char *v, char *buf, size_t cap) {
    const char *e = strchr(v, ';');
    size_t len = e ? (size_t)(e - v) : strlen(v);
    if (len >= cap) len = cap - 1;
    memcpy(buf, v, len);
    buf[len] = 0;
}

// [b, e) of the text split into `parts` pieces that start right after a '\n'
std::vector<size_t> line_cuts(const char *text, size_t len, int parts) {
    std::vector<size_t> cut{0};
    for (int t = 1; t < parts; t++) {
        size_t c = len * (size_t)t / (size_t)parts;
        const void *nl = c < len ? memchr(text + c, '\n', len - c) : nullptr;
        c = nl ? (size_t)((const char *)nl - text) + 1 : len;
        cut.push_back(std::max(c, cut.back()));
    }
    cut.push_back(len);
    return cut;
}

template <typename F>
void run_parts(int parts, F &&f) {
    if (parts <= 1) { f(0); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < parts; t++) th.emplace_back([&, t] { f(t); });
    for (auto &x : th) x.join();
}

}  // namespace

struct svth_vcf {
    std::vector<svt_locus> loci;
    std::string msgs;
};

extern "C" {

// One logical VCF line of process_vcf's reader (audit.c:299-327) -> o.
static void vcf_take(char *line, svth_vcf &o, char *perr, size_t cap) {
    svt_locus l;
    const int act = svth_parse_line(line, &l, perr, cap);
    if (act == 2) o.msgs += perr;
    if (act != 1) return;
    if (svth_is_unknown_type(&l)) o.msgs += "[ERROR] Unkown type.\n";
    o.loci.push_back(l);
}

// The reader loop of audit.c:294-327 exactly, sequentially: fgets into a buffer of current_size
// bytes (1 MiB, doubled whenever a line fills it, never shrunk), strlen (a line ends at its
// first NUL; the rest of what that fgets read is dropped), a final line without '\n' that exactly
// fills the buffer skipped (the next fgets returns NULL, :317), lines shorter than 2 chars and
// '#' lines skipped.  Used when the file has a line of 1 MiB or more (the buffer's history
// matters then); svth_vcf_parse's threaded loop is the same for every shorter line.
static void vcf_parse_exact(const char *text, size_t len, svth_vcf &o) {
    size_t cur = 1u << 20, pos = 0;
    std::string buf(cur, '\0');
    char perr[1024];
    // fgets(buf + at, cap): up to cap - 1 chars through the first '\n'; false (NULL) at the end
    auto fgets_at = [&](size_t at, size_t cap) {
        if (pos >= len) return false;
        const size_t room = std::min(cap - 1, len - pos);
        const void *nl = memchr(text + pos, '\n', room);
        const size_t k = nl ? (size_t)((const char *)nl - (text + pos)) + 1 : room;
        memcpy(&buf[at], text + pos, k);
        buf[at + k] = '\0';
        pos += k;
        return true;
    };
    while (fgets_at(0, cur)) {
        size_t n = strlen(buf.c_str());
        bool skip = false;
        while (n == cur - 1 && buf[n - 1] != '\n') {   // audit.c:304-319
            cur *= 2;
            buf.resize(cur);
            if (!fgets_at(n, cur - n)) { skip = true; break; }
            n = strlen(buf.c_str());
        }
        if (skip || n < 2 || buf[0] == '#') continue;   // :321-322
        if (buf[n - 1] == '\n') n--;                     // :324-327
        std::string line(buf.data(), n);
        vcf_take(&line[0], o, perr, sizeof perr);
    }
}

svth_vcf *svth_vcf_parse(const char *text, size_t len, int threads) {
    const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(threads, 1), len / (1u << 20) + 1));
    const std::vector<size_t> cut = line_cuts(text, len, T);
    std::vector<svth_vcf> part((size_t)T);
    std::atomic<bool> long_line{false};
    run_parts(T, [&](int t) {
        svth_vcf &o = part[(size_t)t];
        std::string line;
        char perr[1024];
        for (size_t i = cut[(size_t)t], e = cut[(size_t)t + 1]; i < e;) {
            const void *nl = memchr(text + i, '\n', e - i);
            const size_t n = (nl ? (size_t)((const char *)nl - text) + 1 : e) - i;
            const char *ln = text + i;
            i += n;
            // a physical line of 1 MiB - 1 chars or more: the reader's buffer history decides
            // (vcf_parse_exact); shorter ones are one fgets each
            if (n >= (1u << 20) - 1) { long_line = true; return; }
            const void *z = memchr(ln, '\0', n);               // strlen: the line ends at a NUL
            const size_t m = z ? (size_t)((const char *)z - ln) : n;
            if (m < 2 || ln[0] == '#') continue;                     // audit.c:321-322
            line.assign(ln, ln[m - 1] == '\n' ? m - 1 : m);         // :324-327
            vcf_take(&line[0], o, perr, sizeof perr);
        }
    });
    svth_vcf *v = new svth_vcf();
    if (long_line) {
        vcf_parse_exact(text, len, *v);
        return v;
    }
    size_t n = 0;
    for (auto &p : part) n += p.loci.size();
    v->loci.reserve(n);
    for (auto &p : part) {
        v->loci.insert(v->loci.end(), p.loci.begin(), p.loci.end());
        v->msgs += p.msgs;
    }
    return v;
}

size_t svth_vcf_count(const svth_vcf *v) { return v->loci.size(); }
const svt_locus *svth_vcf_loci(const svth_vcf *v) { return v->loci.data(); }
const char *svth_vcf_messages(const svth_vcf *v, size_t *len) {
    if (len) *len = v->msgs.size();
    return v->msgs.c_str();
}
void svth_vcf_free(svth_vcf *v) { delete v; }

char *svth_format_batch(const svt_locus *l, const svt_result *r, size_t n, int threads, size_t *len) {
    const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(threads, 1), n / 16384 + 1));
    std::vector<std::string> part((size_t)T);
    run_parts(T, [&](int t) {
        std::string &o = part[(size_t)t];
        const size_t b = n * (size_t)t / (size_t)T, e = n * (size_t)(t + 1) / (size_t)T;
        o.reserve((e - b) * 128);
        char buf[512];
        for (size_t k = b; k < e; k++) {
            const int m = svth_format(&l[k], &r[k], buf, sizeof buf);
            if (m > 0) o.append(buf, (size_t)m);
        }
    });
    size_t tot = 0;
    for (auto &p : part) tot += p.size();
    char *out = (char *)malloc(tot + 1);
    if (!out) return nullptr;
    size_t at = 0;
    for (auto &p : part) { memcpy(out + at, p.data(), p.size()); at += p.size(); }
    out[tot] = 0;
    if (len) *len = tot;
    return out;
}

char *svth_format_evidence(const svt_locus *l, const svt_result *r, const svt_evidence *ev, size_t n, int header,
                           int threads, size_t *len) {
    const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(threads, 1), n / 16384 + 1));
    std::vector<std::string> part((size_t)T);
    run_parts(T, [&](int t) {
        std::string &o = part[(size_t)t];
        const size_t b = n * (size_t)t / (size_t)T, e = n * (size_t)(t + 1) / (size_t)T;
        o.reserve((e - b) * 96);
        char buf[256];
        auto na = [&](uint32_t v, char sep) {   // NA for 0xFFFFFFFF
            const int m = v == SVT_NA ? snprintf(buf, sizeof buf, "NA%c", sep) : snprintf(buf, sizeof buf, "%u%c", v, sep);
            o.append(buf, (size_t)m);
        };
        for (size_t k = b; k < e; k++) {
            const int m = snprintf(buf, sizeof buf, "%zu\t%d\t%d\t%u\t%u\t", k, l[k].type, l[k].chrom, l[k].pos, l[k].end);
            o.append(buf, (size_t)m);
            na(r[k].start, '\t');
            na(r[k].end, '\t');
            for (int w = 0; w < 2; w++) {
                const svt_evidence &x = ev[2 * k + (size_t)w];
                const int q = snprintf(buf, sizeof buf, "%u\t%u\t", x.support, x.depth);
                o.append(buf, (size_t)q);
                na(x.lo, '\t');
                na(x.hi, w ? '\n' : '\t');
            }
        }
    });
    static const char head[] = "#row\ttype\tchrom\tpos\tend\tref_pos\tref_end\tsup_pos\tdepth_pos\tlo_pos\thi_pos\t"
                               "sup_end\tdepth_end\tlo_end\thi_end\n";
    const size_t hl = header ? sizeof head - 1 : 0;
    size_t tot = hl;
    for (auto &p : part) tot += p.size();
    char *out = (char *)malloc(tot + 1);
    if (!out) return nullptr;
    memcpy(out, head, hl);
    size_t at = hl;
    for (auto &p : part) { memcpy(out + at, p.data(), p.size()); at += p.size(); }
    out[tot] = 0;
    if (len) *len = tot;
    return out;
}

char *svth_format_calls(const svt_call *c, size_t n, const char *const *names, size_t n_names, int header, int threads,
                        size_t *len) {
    return svth_format_calls_gt(c, nullptr, n, names, n_names, nullptr, header, threads, len);
}

char *svth_format_calls_gt(const svt_call *c, const svt_gt *gts, size_t n, const char *const *names, size_t n_names,
                           const char *sample, int header, int threads, size_t *len) {
    return svth_format_calls_seq(c, gts, nullptr, nullptr, 0, n, names, n_names, sample, header, threads, len);
}

char *svth_format_calls_seq(const svt_call *c, const svt_gt *gts, const svt_poa_result *cons, const uint8_t *bases, int32_t cap,
                            size_t n, const char *const *names, size_t n_names, const char *sample, int header, int threads,
                            size_t *len) {
    return svth_format_calls_rearr(c, gts, cons, bases, cap, n, names, n_names, sample, header, threads, 0u, len);
}

char *svth_format_calls_rearr(const svt_call *c, const svt_gt *gts, const svt_poa_result *cons, const uint8_t *bases, int32_t cap,
                              size_t n, const char *const *names, size_t n_names, const char *sample, int header, int threads,
                              uint32_t rearr, size_t *len) {
    return svth_format_calls_bnd(c, gts, cons, bases, cap, n, names, n_names, sample, header, threads, rearr, 0u, len);
}

char *svth_format_calls_bnd(const svt_call *c, const svt_gt *gts, const svt_poa_result *cons, const uint8_t *bases, int32_t cap,
                            size_t n, const char *const *names, size_t n_names, const char *sample, int header, int threads,
                            uint32_t rearr, uint32_t bnd, size_t *len) {
    const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(threads, 1), n / 16384 + 1));
    // a call's class: 0 DEL, 1 INS (and every type not asked for, as ever), 2 DUP, 3 INV (rearr != 0), 4 BND (bnd != 0)
    auto cls = [rearr, bnd](const svt_call &x) {
        if (x.type == SVT_DEL) return 0;
        if (rearr && x.type == SVT_DUP) return 2;
        if (rearr && x.type == SVT_INV) return 3;
        if (bnd && x.type == SVT_BND) return 4;
        return 1;
    };
    constexpr int NC = 5;
    static const char *const TY[NC] = {"DEL", "INS", "DUP", "INV", "BND"};
    // the ID's k: the call's rank among the calls of its type (1-based)
    std::vector<size_t> first_k((size_t)T * NC + NC, 0);
    for (int t = 0; t < T; t++) {
        size_t cnt[NC] = {0, 0, 0, 0, 0};
        for (size_t k = n * (size_t)t / (size_t)T, e = n * (size_t)(t + 1) / (size_t)T; k < e; k++) cnt[cls(c[k])]++;
        for (int q = 0; q < NC; q++) first_k[NC * (size_t)t + NC + (size_t)q] = first_k[NC * (size_t)t + (size_t)q] + cnt[q];
    }
    std::vector<std::string> part((size_t)T);
    run_parts(T, [&](int t) {
        std::string &o = part[(size_t)t];
        const size_t b = n * (size_t)t / (size_t)T, e = n * (size_t)(t + 1) / (size_t)T;
        o.reserve((e - b) * 160);
        size_t rank[NC];
        for (int q = 0; q < NC; q++) rank[q] = first_k[NC * (size_t)t + (size_t)q];
        char buf[320], num[16], num2[16];
        for (size_t k = b; k < e; k++) {
            const svt_call &x = c[k];
            const int cl = cls(x);
            const bool del = cl == 0;
            const char *ty = TY[cl];
            const char *name = num;
            if (x.chrom >= 1 && (size_t)x.chrom <= n_names && names && names[x.chrom - 1]) name = names[x.chrom - 1];
            else snprintf(num, sizeof num, "%d", x.chrom);
            o += name;
            int m = snprintf(buf, sizeof buf, "\t%u\tsvtrek.%s.%zu\tN\t", x.pos, ty, ++rank[cl]);
            o.append(buf, (size_t)m);
            if (cl == 4) {   // one record a breakend pair: ALT by o = 2 * s_lo + s_hi, the partner named as CHROM is
                const int32_t mc = SVT_CALL_MATE_CHROM(x);
                const uint32_t ori = SVT_CALL_MATE_ORIENT(x);
                const char *mate = num2;
                if (mc >= 1 && (size_t)mc <= n_names && names && names[mc - 1]) mate = names[mc - 1];
                else snprintf(num2, sizeof num2, "%d", mc);
                const char br = ori & 1u ? '[' : ']';
                if (!(ori & 2u)) o += 'N';
                o += br;
                o += mate;
                m = snprintf(buf, sizeof buf, ":%u%c", x.end, br);
                o.append(buf, (size_t)m);
                if (ori & 2u) o += 'N';
                o += "\t.\tPASS\tSVTYPE=BND;CHR2=";
                o += mate;
                m = snprintf(buf, sizeof buf, ";POS2=%u;SUPPORT=%u;DEPTH=%u;XRANGE=%u,%u;X2RANGE=%u,%u", x.end, x.support, x.depth, x.x_lo,
                             x.x_hi, x.len_lo, x.len_hi);
                o.append(buf, (size_t)m);
                if (gts) o += "\tGT:GQ:DR:DV:PL\t./.:0:0:0:0,0,0";   // (never genotyped)
                o += '\n';
                continue;
            }
            const bool ins_cons = cons && cl == 1;
            if (ins_cons && cons[k].len >= 1 && cons[k].len <= cap && bases) {   // ALT: the base before + the consensus
                const uint8_t *q = bases + k * (size_t)cap;
                o += 'N';
                for (int32_t i = 0; i < cons[k].len; i++) o += "ACGTN"[q[i] < 4 ? q[i] : 4];
            } else {
                o += '<';
                o += ty;
                o += '>';
            }
            m = snprintf(buf, sizeof buf, "\t.\tPASS\tSVTYPE=%s;END=%u;SVLEN=%s%u;SUPPORT=%u;DEPTH=%u;XRANGE=%u,%u;LENRANGE=%u,%u",
                         ty, x.end, del ? "-" : "", x.len, x.support, x.depth, x.x_lo, x.x_hi, x.len_lo, x.len_hi);
            o.append(buf, (size_t)m);
            if (ins_cons) {
                m = snprintf(buf, sizeof buf, ";CONSLEN=%d;CONSREADS=%d", cons[k].len > 0 ? cons[k].len : 0, cons[k].n_used);
                o.append(buf, (size_t)m);
            }
            if (gts) {
                const svt_gt &g = gts[k];
                static const char *const GT[3] = {"0/0", "0/1", "1/1"};
                const int q = g.gt < 0 || g.gt > 2
                                  ? snprintf(buf, sizeof buf, "\tGT:GQ:DR:DV:PL\t./.:0:0:0:0,0,0")
                                  : snprintf(buf, sizeof buf, "\tGT:GQ:DR:DV:PL\t%s:%u:%u:%u:%u,%u,%u", GT[g.gt], g.gq, g.ref, g.alt,
                                             (unsigned)g.pl[0], (unsigned)g.pl[1], (unsigned)g.pl[2]);
                o.append(buf, (size_t)q);
            }
            o += '\n';
        }
    });
    std::string head;
    if (header) {
        head = "##fileformat=VCFv4.2\n##source=svtrek_amd call\n";
        for (size_t t = 0; t < n_names; t++) head += std::string("##contig=<ID=") + (names && names[t] ? names[t] : "") + ">\n";
        head += "##ALT=<ID=DEL,Description=\"Deletion\">\n##ALT=<ID=INS,Description=\"Insertion\">\n";
        if (rearr & (1u << SVT_DUP)) head += "##ALT=<ID=DUP,Description=\"Tandem duplication\">\n";
        if (rearr & (1u << SVT_INV)) head += "##ALT=<ID=INV,Description=\"Inversion\">\n";
        head += "##INFO=<ID=SVTYPE,Number=1,Type=String,Description=\"Type of structural variant\">\n"
                "##INFO=<ID=END,Number=1,Type=Integer,Description=\"DEL: rounded mean of the ops' walk end + 1; INS: POS + 1\">\n"
                "##INFO=<ID=SVLEN,Number=1,Type=Integer,Description=\"Rounded mean length of the supporting ops (negative: DEL)\">\n"
                "##INFO=<ID=SUPPORT,Number=1,Type=Integer,Description=\"CIGAR ops in the cluster\">\n"
                "##INFO=<ID=DEPTH,Number=1,Type=Integer,Description=\"Reads covering POS\">\n"
                "##INFO=<ID=XRANGE,Number=2,Type=Integer,Description=\"Smallest and largest start of the supporting ops\">\n"
                "##INFO=<ID=LENRANGE,Number=2,Type=Integer,Description=\"Smallest and largest length of the supporting ops\">\n";
        if (bnd)
            head += "##INFO=<ID=CHR2,Number=1,Type=String,Description=\"BND: the partner breakend's contig\">\n"
                    "##INFO=<ID=POS2,Number=1,Type=Integer,Description=\"BND: rounded mean of the partner breakend's position\">\n"
                    "##INFO=<ID=X2RANGE,Number=2,Type=Integer,Description=\"BND: smallest and largest partner position of the supporting reads\">\n";
        if (cons)
            head += "##INFO=<ID=CONSLEN,Number=1,Type=Integer,Description=\"INS: length of the consensus inserted sequence (0: none)\">\n"
                    "##INFO=<ID=CONSREADS,Number=1,Type=Integer,Description=\"INS: inserted sequences fused into the consensus\">\n";
        if (gts)
            head += "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
                    "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype quality: the smaller PL of the other two genotypes, at most 99\">\n"
                    "##FORMAT=<ID=DR,Number=1,Type=Integer,Description=\"Spanning reads without a supporting op\">\n"
                    "##FORMAT=<ID=DV,Number=1,Type=Integer,Description=\"Spanning reads' supporting ops\">\n"
                    "##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"Phred-scaled genotype likelihoods, rounded\">\n";
        head += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO";
        if (gts) head += std::string("\tFORMAT\t") + (sample && sample[0] ? sample : "SAMPLE");
        head += '\n';
    }
    size_t tot = head.size();
    for (auto &p : part) tot += p.size();
    char *out = (char *)malloc(tot + 1);
    if (!out) return nullptr;
    memcpy(out, head.data(), head.size());
    size_t at = head.size();
    for (auto &p : part) { memcpy(out + at, p.data(), p.size()); at += p.size(); }
    out[tot] = 0;
    if (len) *len = tot;
    return out;
}

void svth_free(void *p) { free(p); }

int svth_parse_line(char *line, svt_locus *l, char *err, size_t errcap) {
    char *save = nullptr, *alt_save = nullptr;
    if (err && errcap) err[0] = 0;
    char *chrom = strtok_r(line, "\t", &save);
    char *index = strtok_r(nullptr, "\t", &save);
    if (!index) {
        if (err) snprintf(err, errcap, "VCF: no index at line: %s\n", line);
        return 2;
    }
    strtok_r(nullptr, "\t", &save);                       // ID
    char *seq = strtok_r(nullptr, "\t", &save);           // REF
    char *alt = seq ? strtok_r(nullptr, "\t", &save) : nullptr;
    if (!seq || !alt) {   // the reference dereferences NULL here; report and skip instead
        if (err) snprintf(err, errcap, "VCF: truncated record at POS %s\n", index);
        return 2;
    }
    size_t seq_len = strlen(seq), max_alt = 0, min_alt = 0x7FFFFFFF;
    for (char *t = strtok_r(alt, ",", &alt_save); t; t = strtok_r(nullptr, ",", &alt_save)) {
        size_t k = strlen(t);
        if (k > max_alt) max_alt = k;
        if (k < min_alt) min_alt = k;
    }
    strtok_r(nullptr, "\t", &save);                       // QUAL
    strtok_r(nullptr, "\t", &save);                       // FILTER
    char *info = strtok_r(nullptr, "\t", &save);          // INFO
    if (!info) {
        if (err) snprintf(err, errcap, "VCF: truncated record at POS %s\n", index);
        return 2;
    }
    int chrom_index = strncmp(chrom, "chr", 3) == 0 ? atoi(chrom + 3) : atoi(chrom);
    uint32_t pos = (uint32_t)strtol(index, nullptr, 10);
    if (pos == 0 && index[0] != '0') {
        if (err) snprintf(err, errcap, "[ERROR] Conversion error to pos %s\n", index);
        return 2;
    }
    int type;
    if (const char *sv = strstr(info, "SVTYPE=")) {
        char b[16];
        info_value(sv + 7, b, sizeof b);
        type = sv_type_of(b);
    } else if (seq_len == 1 && (size_t)SV_MIN_LENGTH < max_alt) {
        type = SVT_INS;
    } else if ((size_t)SV_MIN_LENGTH < seq_len && min_alt == 1) {
        type = SVT_DEL;
    } else {
        return 0;
    }
    uint32_t end;
    if (const char *es = strstr(info, "END=")) {
        char b[32];
        info_value(es + 4, b, sizeof b);
        end = (uint32_t)strtol(b, nullptr, 10);
        if (end == 0 && b[0] != '0') return 0;
    } else {
        end = pos + (uint32_t)seq_len;
    }
    if ((type == SVT_DEL || type == SVT_INV) && end - pos < (uint32_t)SV_MIN_LENGTH) return 0;
    l->type = type;
    l->chrom = chrom_index;
    l->pos = pos;
    l->end = end;
    return 1;
}

int svth_is_unknown_type(const svt_locus *l) {
    return !(l->type == SVT_INS || l->type == SVT_DEL || l->type == SVT_INV);
}

int svth_format(const svt_locus *l, const svt_result *r, char *buf, size_t cap) {
    const uint32_t pos = l->pos, end = l->end;
    buf[0] = 0;
    if (l->type == SVT_INS) {
        if (r->start == SVT_NA)
            return snprintf(buf, cap, "(INS) chr: %d, org pos: %u, ref pos: NA\n", l->chrom, pos);
        return snprintf(buf, cap, "(INS) chr: %d, org pos: %u, ref pos: %u, diff: %d\n", l->chrom, pos, r->start,
                        (int)(r->start - pos));
    }
    if (l->type == SVT_DEL) {
        if (!((uint32_t)SV_MIN_LENGTH < end - pos)) return 0;
        int n = snprintf(buf, cap, "(DEL) chr: %d, org pos: %u, org end: %u, ref pos: ", l->chrom, pos, end);
        auto put = [&](const char *fmt, long v) { n += snprintf(buf + n, cap - (size_t)n, fmt, v); };
        if (r->start == SVT_NA) n += snprintf(buf + n, cap - (size_t)n, "NA, ref end: ");
        else put("%ld, ref end: ", (long)(int)r->start);
        if (r->end == SVT_NA) n += snprintf(buf + n, cap - (size_t)n, "NA, ");
        else put("%ld, ", (long)(int)r->end);
        if (r->start == SVT_NA) n += snprintf(buf + n, cap - (size_t)n, "diff pos: NA, ");
        else put("diff pos: %ld, ", (long)(int)(r->start - pos));
        if (r->end == SVT_NA) n += snprintf(buf + n, cap - (size_t)n, "diff end: NA\n");
        else put("diff end: %ld\n", (long)(int)(r->end - end));
        return n;
    }
    if (l->type == SVT_INV) {
        if (!((uint32_t)SV_MIN_LENGTH < end - pos)) return 0;
        return snprintf(buf, cap, "(INV) chr: %d, org pos: %u, org end: %u, ref pos: %u, ref end: %u\n", l->chrom,
                        pos, end, r->start, r->end);
    }
    return 0;
}

}  // extern "C"
