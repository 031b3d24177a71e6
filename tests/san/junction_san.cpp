// Sanitizer driver for the SA ingest of bam_ingest.cpp (svth_bam_read_sa, svth_bam_junctions): built with
// ASan+UBSan by tests/test_junction_san.py and run on the BAMs of tests/test_junction_ingest.py, the
// malformed ones included.  Prints the segment table, one line per row, for the test to compare with the
// uninstrumented library's.
//   junction_san BAM THREADS [tid0 beg0 tid1 end1]
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "svtrek_host.h"

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const int T = atoi(argv[2]);
    char err[512];
    svth_bam *b = argc >= 7 ? svth_bam_read_sa(argv[1], T, atoi(argv[3]), atoll(argv[4]), atoi(argv[5]), atoll(argv[6]), nullptr, err,
                                               sizeof err)
                            : svth_bam_read_sa(argv[1], T, -1, 0, -1, 0, nullptr, err, sizeof err);
    if (!b) { fprintf(stderr, "bam: %s\n", err); return 1; }
    svt_junction_view v;
    if (!svth_bam_junctions(b, &v)) { fprintf(stderr, "no table\n"); return 1; }
    svt_pileup_view p;
    svth_bam_view(b, &p);
    printf("reads %lld records %llu malformed %lld\n", (long long)(p.n_targets ? p.tid_off[p.n_targets] : 0),
           (unsigned long long)v.n, (long long)svth_bam_n_sa_malformed(b));
    for (uint64_t k = 0; k < v.n; k++)
        for (uint64_t r = v.off[k]; r < v.off[k + 1]; r++) {
            const svt_junction_seg &s = v.seg[r];
            printf("%llu %d %u %u %u %u %u\n", (unsigned long long)v.read[k], s.tid, s.strand, s.r_beg, s.r_end, s.q_beg, s.q_end);
        }
    svth_bam_free(b);
    return 0;
}
