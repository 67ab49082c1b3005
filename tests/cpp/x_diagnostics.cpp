// PLS::Model::x_diagnostics (include/PLS/pls.h) against the definitions evaluated here on the host from the model's own
// public scores and loadings: Q residuals, Hotelling T^2, R^2 X for 1..A components, on the training data and on a block
// of rows taken as new data, after a KERNEL_TYPE1 and a KERNEL_TYPE2 fit and after a refit through plsr().
// This checks the wiring of the C++ layer (which matrix, which component, which rows, tvar of the TRAINING scores) with the
// project's parity bar of 1e-10 on the scale of a row's arithmetic; the rounding-level bars are those of tests/test_gpu_xdiag.py.
// Usage: x_diagnostics X.csv Y.csv ncomp      prints "x_diagnostics: ok" and returns 0, or says what differs.
#include <PLS/pls.h>

#include <cmath>
#include <cstdlib>
#include <iostream>
#include <vector>

namespace {

int failures = 0;

void expect(bool ok, const char *what, long i, long c, double got, double want, double bar) {
    if (ok) return;
    if (failures++ < 8)
        std::cout << what << "[" << i << "," << c << "]: got " << got << " want " << want << " bar " << bar << "\n";
}

// the definitions, from S = X R and P; tvar from the training scores St
void check(const char *label, const PLS::Model &m, const Mat2D &X, const Mat2D &St, size_t A) {
    const long N = X.rows(), K = X.cols(), Ai = static_cast<long>(A), Nt = St.rows();
    const PLS::XDiagnostics d = m.x_diagnostics(X);
    const Mat2Dc Sc = m.scores(X), Pc = m.loadingsX();
    if (d.Q.rows() != N || d.Q.cols() != Ai || d.T2.rows() != N || d.T2.cols() != Ai || d.R2X.size() != Ai) {
        std::cout << label << ": wrong shapes\n";
        ++failures;
        return;
    }
    std::vector<double> tvar(A), ssx(A + 1, 0.0), bssx(A + 1, 0.0);
    for (long a = 0; a < Ai; ++a) {
        double tt = 0;
        for (long i = 0; i < Nt; ++i) tt += St(i, a) * St(i, a);
        tvar[a] = tt / (Nt - 1);
    }
    // scale of a row's residual arithmetic: ||x_i|| + sum_a |s_ia| ||p_a||
    std::vector<double> pn(A);
    for (long a = 0; a < Ai; ++a) {
        double s = 0;
        for (long k = 0; k < K; ++k) s += std::real(Pc(k, a)) * std::real(Pc(k, a));
        pn[a] = std::sqrt(s);
    }
    std::vector<double> f(static_cast<size_t>(K));
    for (long i = 0; i < N; ++i) {
        double x2 = 0, t2 = 0, envt = 0, env = 0;
        for (long k = 0; k < K; ++k) { f[k] = X(i, k); x2 += f[k] * f[k]; }
        ssx[0] += x2;
        env = std::sqrt(x2);
        for (long c = 0; c < Ai; ++c) {
            const double s = std::real(Sc(i, c));
            double q = 0;
            for (long k = 0; k < K; ++k) { f[k] -= s * std::real(Pc(k, c)); q += f[k] * f[k]; }
            env += std::fabs(s) * pn[c];
            t2 += s * s / tvar[c];
            envt += s * s / tvar[c];
            const double bq = 1e-10 * env * env, bt = 1e-9 * (1.0 + envt);
            expect(std::fabs(d.Q(i, c) - q) <= bq, "Q", i, c, d.Q(i, c), q, bq);
            expect(std::fabs(d.T2(i, c) - t2) <= bt, "T2", i, c, d.T2(i, c), t2, bt);
            ssx[c + 1] += q;
            bssx[c + 1] += bq;
        }
    }
    for (long c = 0; c < Ai; ++c) {
        const double want = 1.0 - ssx[c + 1] / ssx[0];
        const double bar = bssx[c + 1] / ssx[0] + 1e-10;
        expect(std::fabs(d.R2X[c] - want) <= bar, "R2X", 0, c, d.R2X[c], want, bar);
    }
    std::cout << label << ": R2X(A) = " << d.R2X[Ai - 1] << "\n";
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 4) return 100;
    const Mat2D X = PLS::colwise_z_scores(PLS::read_matrix_file(argv[1]));
    const Mat2D Y = PLS::colwise_z_scores(PLS::read_matrix_file(argv[2]));
    const size_t A = static_cast<size_t>(std::atoi(argv[3]));
    const long N = X.rows(), nnew = std::max<long>(1, N / 4);
    Mat2D Xnew(nnew, X.cols());  // the last rows, taken as new data
    for (long k = 0; k < X.cols(); ++k)
        for (long i = 0; i < nnew; ++i) Xnew(i, k) = X(N - nnew + i, k);
    for (int method = 0; method < 2; ++method) {
        PLS::Model m(X, Y, method == 0 ? PLS::KERNEL_TYPE1 : PLS::KERNEL_TYPE2, A);
        Mat2D St(N, static_cast<long>(A));
        {
            const Mat2Dc s = m.scores(X);
            for (long j = 0; j < St.cols(); ++j)
                for (long i = 0; i < N; ++i) St(i, j) = std::real(s(i, j));
        }
        check(method == 0 ? "KERNEL_TYPE1 training" : "KERNEL_TYPE2 training", m, X, St, A);
        check(method == 0 ? "KERNEL_TYPE1 new rows" : "KERNEL_TYPE2 new rows", m, Xnew, St, A);
        // on training data the T2 of c components sum to c (N - 1)
        const PLS::XDiagnostics d = m.x_diagnostics(X);
        for (long c = 0; c < static_cast<long>(A); ++c) {
            double t = 0;
            for (long i = 0; i < N; ++i) t += d.T2(i, c);
            expect(std::fabs(t - (c + 1.0) * (N - 1)) <= 1e-10 * (c + 1) * N, "sum T2", 0, c, t, (c + 1.0) * (N - 1), 1e-10 * (c + 1) * N);
        }
        // a refit through plsr() on the same data leaves the same diagnostics (tvar is taken at the fit: the data is not kept)
        m.plsr(X, Y, method == 0 ? PLS::KERNEL_TYPE1 : PLS::KERNEL_TYPE2);
        const PLS::XDiagnostics d2 = m.x_diagnostics(Xnew), d1 = PLS::Model(X, Y, method == 0 ? PLS::KERNEL_TYPE1 : PLS::KERNEL_TYPE2, A).x_diagnostics(Xnew);
        for (long c = 0; c < static_cast<long>(A); ++c)
            for (long i = 0; i < nnew; ++i) {
                expect(d1.Q(i, c) == d2.Q(i, c), "Q after plsr", i, c, d2.Q(i, c), d1.Q(i, c), 0);
                expect(d1.T2(i, c) == d2.T2(i, c), "T2 after plsr", i, c, d2.T2(i, c), d1.T2(i, c), 0);
            }
    }
    if (failures) {
        std::cout << "x_diagnostics: " << failures << " differences\n";
        return 1;
    }
    std::cout << "x_diagnostics: ok\n";
    return 0;
}
