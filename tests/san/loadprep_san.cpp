// loadprep_san.cpp -- the load's host pass (svtrek_amd/csrc/svt_loadprep.h) as a stand-alone program for the
// sanitizers: the seeded run of tests/native/loadprep_shim.cpp, its digests on stdout.
//   loadprep_san SEED THREADS
#include <stdlib.h>

#include "../native/loadprep_shim.cpp"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    static char text[8192];
    if (lp_seeded_digest(strtoull(argv[1], nullptr, 10), atoi(argv[2]), text, (int)sizeof text) < 0) return 1;
    fputs(text, stdout);
    return 0;
}
