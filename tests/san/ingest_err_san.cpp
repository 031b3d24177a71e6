// Sanitizer driver for the error exits of the host BAM reader (bam_ingest.cpp): built with ASan+UBSan by
// svtrek_amd.build.build_sanitizers, run by tests/test_ingest_err_san.py on the crafted files of
// tests/test_ingest_errors.py with the leak checker on.  Every reader is called on the one path; each prints
// its error, or "ok".
//   ingest_err_san BAM THREADS [tid0 beg0 tid1 end1]
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "svtrek_host.h"

static int sink_begin(void *, int32_t, char *, size_t) { return 0; }
static int sink_feed(void *, const uint8_t *, size_t, const svt_bgzf_block *, size_t, uint64_t, char *, size_t) { return 0; }

static void report(const char *entry, svth_bam *b, const char *err) {
    printf("%s: %s\n", entry, b ? "ok" : err);
    svth_bam_free(b);
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const char *path = argv[1];
    const int T = atoi(argv[2]);
    const bool region = argc >= 7;
    const int32_t t0 = region ? atoi(argv[3]) : -1, t1 = region ? atoi(argv[5]) : -1;
    const int64_t b0 = region ? atoll(argv[4]) : 0, e1 = region ? atoll(argv[6]) : 0;
    char err[512] = {0};
    if (!region) report("read", svth_bam_read(path, T, err, sizeof err), err);
    report("region", svth_bam_read_region(path, T, t0, b0, t1, e1, err, sizeof err), err);
    report("seq", svth_bam_read_seq(path, T, t0, b0, t1, e1, nullptr, err, sizeof err), err);
    report("sa", svth_bam_read_sa(path, T, t0, b0, t1, e1, nullptr, err, sizeof err), err);
    if (!region) {   // (the device path reads whole files)
        svth_dev_sink sink{};
        sink.begin = sink_begin;
        sink.feed = sink_feed;
        sink.batch_bytes = 100;
        int32_t n_targets = 0;
        const int rc = svth_bam_read_device(path, T, &sink, &n_targets, nullptr, err, sizeof err);
        printf("device: %s\n", rc ? err : "ok");
    }
    return 0;
}
