// PLS::Model::permutation_test (include/PLS/pls.h, on pls_hip_fit_batch) against the member functions of one
// Model(X, Y_b, KERNEL_TYPE2, A) per problem: R^2 Y of c components = 1 - SSE_c / SST from Model::SSE, for Y itself and
// for every permuted Y, and the p-values counted from those.
// This checks the wiring of the C++ layer (which rows, which problem, which component); the bar is the project's Gram-route
// parity bar of 1e-8 (both sides work on X^T X); the rounding-level bars are those of tests/test_gpu_fit_batch.py.
// Usage: fit_batch X.csv Y.csv ncomp nperm      prints "fit_batch: ok" and returns 0, or says what differs.
#include <PLS/pls.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <numeric>
#include <random>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 5) return 100;
    const Mat2D X = PLS::colwise_z_scores(PLS::read_matrix_file(argv[1]));
    const Mat2D Y = PLS::colwise_z_scores(PLS::read_matrix_file(argv[2]));
    const size_t A = static_cast<size_t>(std::atoi(argv[3]));
    const int nperm = std::atoi(argv[4]);
    const long N = X.rows(), M = Y.cols(), Ai = static_cast<long>(A);
    std::mt19937 rng(20261016u);
    std::vector<Colsz> perms;
    for (int b = 0; b < nperm; ++b) {
        std::vector<size_t> idx(static_cast<size_t>(N));
        std::iota(idx.begin(), idx.end(), size_t(0));
        std::shuffle(idx.begin(), idx.end(), rng);
        Colsz p(N);
        for (long i = 0; i < N; ++i) p(i) = idx[static_cast<size_t>(i)];
        perms.push_back(p);
    }
    const PLS::Model model(X, Y, PLS::KERNEL_TYPE2, A);
    const PLS::PermutationTest t = model.permutation_test(X, Y, perms);
    int failures = 0;
    if (t.r2y.rows() != M || t.r2y.cols() != Ai || static_cast<int>(t.r2y_perm.size()) != nperm || t.p.rows() != M || t.p.cols() != Ai) {
        std::cout << "fit_batch: wrong shapes\n";
        return 1;
    }
    std::vector<Mat2D> want;  // problem 0: Y itself
    for (int b = 0; b <= nperm; ++b) {
        Mat2D Yb(N, M);
        for (long m = 0; m < M; ++m)
            for (long i = 0; i < N; ++i) Yb(i, m) = b == 0 ? Y(i, m) : Y(static_cast<long>(perms[static_cast<size_t>(b - 1)](i)), m);
        const PLS::Model mb(X, Yb, PLS::KERNEL_TYPE2, A);
        const Row sst = PLS::SST(Yb);
        Mat2D r2(M, Ai);
        for (long c = 0; c < Ai; ++c) {
            const Row sse = mb.SSE(X, Yb, static_cast<size_t>(c + 1));
            for (long m = 0; m < M; ++m) r2(m, c) = 1.0 - sse[m] / sst[m];
        }
        const Mat2D &got = b == 0 ? t.r2y : t.r2y_perm[static_cast<size_t>(b - 1)];
        for (long c = 0; c < Ai; ++c)
            for (long m = 0; m < M; ++m)
                if (!(std::fabs(got(m, c) - r2(m, c)) <= 1e-8)) {
                    if (failures++ < 8)
                        std::cout << "r2y problem " << b << " [" << m << "," << c << "]: got " << got(m, c) << " want " << r2(m, c) << "\n";
                }
        want.push_back(r2);
    }
    for (long c = 0; c < Ai; ++c)
        for (long m = 0; m < M; ++m) {
            int ge = 0;
            double gap = 1.0;  // a count decided by less than the bar is not a wiring error
            for (int b = 1; b <= nperm; ++b) {
                ge += want[static_cast<size_t>(b)](m, c) >= want[0](m, c) ? 1 : 0;
                gap = std::min(gap, std::fabs(want[static_cast<size_t>(b)](m, c) - want[0](m, c)));
            }
            const double p = (1.0 + ge) / (nperm + 1.0);
            if (gap > 1e-7 && t.p(m, c) != p) {
                if (failures++ < 8) std::cout << "p [" << m << "," << c << "]: got " << t.p(m, c) << " want " << p << "\n";
            }
        }
    std::cout << "R2Y(A) = " << t.r2y(0, Ai - 1) << "  p(A) = " << t.p(0, Ai - 1) << "\n";
    if (failures) {
        std::cout << "fit_batch: " << failures << " differences\n";
        return 1;
    }
    std::cout << "fit_batch: ok\n";
    return 0;
}
