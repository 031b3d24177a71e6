// jnclass_san.cpp -- the junction classifier (svtrek_amd/csrc/svt_jnclass.h) as a stand-alone program for the
// sanitizers: the seeded table and the extreme-value table of tests/native/jnclass_shim.cpp classified, their
// digests on stdout.
//   jnclass_san SEED RECORDS MIN_LEN X_SAT LEN_MAX EXT_MAX
#include <stdlib.h>

#include "../native/jnclass_shim.cpp"

int main(int argc, char **argv) {
    if (argc != 7) return 2;
    const int64_t lim[4] = {atoll(argv[3]), atoll(argv[4]), atoll(argv[5]), atoll(argv[6])};
    static char text[1024];
    if (jc_digest(lim, strtoull(argv[1], nullptr, 10), strtoull(argv[2], nullptr, 10), text, (int)sizeof text) < 0) return 1;
    fputs(text, stdout);
    return 0;
}
