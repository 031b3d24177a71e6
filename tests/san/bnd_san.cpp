// Sanitizer driver for the VCF writer of `svtrek call --breakends` (svth_format_calls_bnd, vcf_audit.cpp): built
// with ASan+UBSan by tests/test_bnd_host.py.  Formats N generated calls of all five types (and one unknown type
// code) for the masks and thread count given, with genotype records when GT is 1, and prints the text for the
// test to compare with the uninstrumented library's.
//   bnd_san N REARR_MASK BND THREADS GT
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "svtrek_host.h"

int main(int argc, char **argv) {
    if (argc < 6) return 2;
    const size_t n = (size_t)atoll(argv[1]);
    const uint32_t rearr = (uint32_t)atoi(argv[2]), bnd = (uint32_t)atoi(argv[3]);
    const int threads = atoi(argv[4]), with_gt = atoi(argv[5]);
    static const int32_t TYPES[6] = {SVT_DEL, SVT_BND, SVT_INS, SVT_INV, SVT_DUP, 5};
    std::vector<svt_call> calls(n);
    std::vector<svt_gt> gts(n + 1);
    for (size_t k = 0; k < n; k++) {   // (tests/test_bnd_host.py generates the same records)
        svt_call &c = calls[k];
        c.type = TYPES[k % 6];
        c.chrom = (int32_t)(1 + (k / 1000) % 4);   // (4: past the two names)
        c.pos = (uint32_t)(100 + 7 * k);
        c.len = c.type == SVT_BND ? 0u : (uint32_t)(50 + k % 977);
        c.end = c.pos + (uint32_t)(50 + k % 977);
        c.support = (uint32_t)(3 + k % 5);
        c.depth = (uint32_t)(k % 60);
        c.len_lo = c.end - 1;
        c.len_hi = c.end + 2;
        c.x_lo = c.pos - 3;
        c.x_hi = c.pos + 4;
        c.pad = c.type == SVT_BND ? (uint32_t)((1 + (k / 7) % 5) << 2 | (k / 6) % 4) : 0u;   // (mates 3 .. 5: past the names)
        svt_gt &g = gts[k];
        g = svt_gt{};
        g.gt = c.type == SVT_DEL || c.type == SVT_INS ? (int32_t)(k % 3) : -1;
        if (g.gt >= 0) {
            g.alt = (uint32_t)(k % 11);
            g.ref = (uint32_t)(k % 7);
            g.gq = (uint32_t)(k % 100);
            g.pl[0] = (uint16_t)(k % 500);
            g.pl[2] = (uint16_t)(k % 300);
        }
    }
    const char *names[2] = {"chr1", "chr2"};
    size_t len = 0;
    char *text = svth_format_calls_bnd(n ? calls.data() : nullptr, with_gt ? gts.data() : nullptr, nullptr, nullptr, 0, n, names, 2,
                                       "S1", 1, threads, rearr, bnd, &len);
    if (!text) return 1;
    fwrite(text, 1, len, stdout);
    svth_free(text);
    return 0;
}
