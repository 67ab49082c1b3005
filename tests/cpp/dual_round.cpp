// The slabs of the sample-space rounds (pls_amd/csrc/dual_layout.hpp) without a GPU: tests/test_dual_round.py.
// stdin, one case per line:  N M A ts nround
// stdout, one line per case and layout:  <layout> <bytes_per_item> <name>:<byte offset of the field from the slab's base> ...
// The slab is allocated with nround * bytes_per_item() bytes and the first and last byte of every field are written, so
// that a field outside it is an AddressSanitizer report.
#include "../../pls_amd/csrc/dual_layout.hpp"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <utility>
#include <vector>

using plsk::i64;
typedef std::vector<std::pair<const char *, int>> Names;  // (name, field index; -1: the trailing int field), any order

static int show(const char *layout, const plsk::ItemLayout &l, i64 nround, const Names &names) {
    if (!l.ok || (int)names.size() != l.n + (l.ints ? 1 : 0)) return 1;  // every field of the layout is named
    const size_t bytes = (size_t)(nround * l.bytes_per_item());
    char *slab = (char *)std::malloc(bytes);
    if (!slab) return 1;
    double *base = (double *)slab;
    std::printf("%s %lld", layout, (long long)l.bytes_per_item());
    for (const auto &f : names) {
        char *p = f.second < 0 ? (char *)l.int_field(base, nround) : (char *)l.field(base, nround, f.second);
        char *q = f.second < 0 ? p + nround * l.ints * 4 : (char *)l.field(base, nround, f.second + 1);  // (field n: the doubles' end)
        p[0] = 1;
        q[-1] = 1;
        std::printf(" %s:%lld", f.first, (long long)(p - slab));
    }
    std::printf("\n");
    std::free(slab);
    return 0;
}

int main() {
    using namespace plsk;
    long long N, M, A, ts, nround;
    while (std::cin >> N >> M >> A >> ts >> nround) {
        int bad = 0;
        bad |= show("cv", cv_dual_layout(N, M, A, ts), nround,
                    {{"Ya", DUAL_YA}, {"Z", DUAL_Z}, {"T", CV_T}, {"tt", CV_TT}, {"scr", CV_SCR}, {"pred", CV_PRED}, {"pos", -1}});
        bad |= show("batch", batch_dual_layout(N, M, A), nround,
                    {{"Ya", DUAL_YA}, {"Z", DUAL_Z}, {"T", BAT_T}, {"U", BAT_U}, {"C", BAT_C}, {"Q", BAT_Q}, {"tt", BAT_TT}, {"scr", BAT_SCR}});
        bad |= show("resample", resample_layout(N, M, A), nround,
                    {{"Ya", DUAL_YA}, {"Z", DUAL_Z}, {"T", BAT_T}, {"U", BAT_U}, {"C", BAT_C}, {"Q", BAT_Q}, {"tt", BAT_TT}, {"scr", BAT_SCR},
                     {"s", RS_S}, {"Yin", RS_YIN}});
        bad |= show("cvbatch", cvbatch_layout(N, M, A, ts), nround,
                    {{"Ya", DUAL_YA}, {"Z", DUAL_Z}, {"T", CV_T}, {"tt", CV_TT}, {"scr", CV_SCR}, {"pred", CV_PRED}, {"yte", CVB_YTE},
                     {"escr", CVB_ESCR}, {"press", CVB_PRESS}, {"ssy", CVB_SSY}});
        if (bad) {
            std::printf("bad layout\n");
            return 1;
        }
    }
    return 0;
}
