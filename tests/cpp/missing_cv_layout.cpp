// The slab of a round of pls_hip_cv_folds_missing (pls_amd/csrc/miss_layout.hpp) without a GPU: tests/test_missing_cv_ref.py.
// stdin, one case per line:  N K M A ts nround es num_cu   (ts is read and echoed only: the test rows live outside the slab)
// stdout, one line per case:  <bytes of a fold> <name>:<byte offset in the fold's slab>:<bytes up to the next field> ...
// The round is allocated with nround * bytes bytes and the first and last byte of every field of every fold are written, so
// that a field outside it is an AddressSanitizer report; a byte written twice is an overlap and fails the run.
#include "../../pls_amd/csrc/miss_layout.hpp"

#include <cstdio>
#include <cstdlib>
#include <iostream>

int main() {
    using namespace plsk;
    static const char *const names[MCV_FIELDS] = {"work", "Ya", "mask", "u", "t", "tm", "tprev", "w", "p", "q", "colpart", "sspart",
                                                  "tpart", "ypart", "yss", "qq", "words"};
    long long N, K, M, A, ts, nround, es, ncu;
    while (std::cin >> N >> K >> M >> A >> ts >> nround >> es >> ncu) {
        const MissCvLayout l = miss_cv_layout(N, K, M, A, (int)es, (int)ncu);
        char *slab = (char *)std::calloc((size_t)(nround * l.bytes), 1);
        if (!slab) return 1;
        for (long long f = 0; f < nround; ++f)
            for (int i = 0; i < MCV_FIELDS; ++i) {
                if (l.off[i + 1] == l.off[i]) continue;  // (an empty field: tpart without a K split)
                char *p = slab + f * l.bytes + l.off[i], *q = slab + f * l.bytes + l.off[i + 1] - 1;
                if (*p || *q) {
                    std::printf("overlap at fold %lld field %s\n", f, names[i]);
                    return 1;
                }
                *p = 1;
                *q = 1;
            }
        std::printf("%lld", (long long)l.bytes);
        for (int i = 0; i < MCV_FIELDS; ++i) std::printf(" %s:%lld:%lld", names[i], (long long)l.off[i], (long long)(l.off[i + 1] - l.off[i]));
        std::printf("\n");
        std::free(slab);
    }
    return 0;
}
