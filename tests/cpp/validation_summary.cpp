// The validation summary behind PLS::validation / PLS::optimal_num_components (formed on the device, pls_hip_validation)
// against a recomputation through the public host functions on Residual::errors(), and cv_NEW_DATA against A separate
// residuals() calls.  tests/test_gpu_validation.py runs it:   validation_summary X.csv Y.csv
//
// Second use, a measurement:           validation_summary --measure M nobs A [reps]
// Synthetic residuals on the device; prints the device time of pls_hip_validation per kernel family over `reps` calls and
// the wall time of the host path it replaces -- the download of E, then the column sums of squares and the std::sort-based
// Wilcoxon loop of pls.cpp with the reference's early exit -- on the same residuals.
#include <PLS/pls.h>
#include <hip/hip_runtime_api.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pls_hip.h"

namespace {

int failures = 0;
void expect(bool ok, const char *what) {
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) ++failures;
}

// the host path of the parent of this feature: plain loops and the public wilcoxon(), early exit at the first hit
Mat2D host_press(const std::vector<Mat2D> &errors) {
    Mat2D out = Mat2D::Zero(static_cast<long>(errors.size()), errors[0].cols());
    for (size_t y = 0; y < errors.size(); ++y)
        for (long c = 0; c < errors[y].cols(); ++c) {
            float_type s = 0;
            for (long i = 0; i < errors[y].rows(); ++i) s += errors[y](i, c) * errors[y](i, c);
            out(static_cast<long>(y), c) = s;
        }
    return out;
}
std::vector<size_t> host_pick(const std::vector<Mat2D> &errors, const Mat2D &press, float_type alpha) {
    std::vector<size_t> best(errors.size());
    for (size_t y = 0; y < errors.size(); ++y) {
        long ref_min = 0;
        for (long c = 1; c < press.cols(); ++c)
            if (press(static_cast<long>(y), c) < press(static_cast<long>(y), ref_min)) ref_min = c;
        long pick = ref_min;
        const Col err_ref = errors[y].col(ref_min);
        for (long alt = 0; alt < ref_min; ++alt)
            if (PLS::wilcoxon(err_ref, errors[y].col(alt)) > alpha) {
                pick = alt;
                break;
            }
        best[y] = static_cast<size_t>(pick) + 1;
    }
    return best;
}

// wilcoxon() of pls.cpp with n (n + 1) (2 n + 1) formed in fp64: the size_t product of the host function (and of the
// reference, src/pls.cpp:208) wraps beyond n = 2.09e6 rows, which inflates its z by 1.78 at n = 3e6
float_type wilcoxon_unwrapped(const Col &err_1, const Col &err_2) {
    const size_t n = static_cast<size_t>(err_1.size());
    std::vector<float_type> mag(n);
    std::vector<int> sign(n);
    for (size_t i = 0; i < n; ++i) {
        const float_type d = std::fabs(err_1[static_cast<long>(i)]) - std::fabs(err_2[static_cast<long>(i)]);
        sign[i] = (0 < d) - (d < 0);
        mag[i] = std::fabs(d);
    }
    const std::vector<size_t> order = PLS::ordered(mag);
    float_type d = 0;
    for (size_t rank = 0; rank < n; ++rank) d += static_cast<float_type>(rank + 1) * sign[order[rank]];
    const float_type nn = static_cast<float_type>(n), t = nn * (nn + 1) / 2.0;
    const float_type sv = std::sqrt(nn * (nn + 1) * (2 * nn + 1) / 24.0);
    return 1.0 - PLS::normalcdf(((t - d) / 2.0 - t / 2.0) / sv);
}

void check_residual(const PLS::Residual &r, const char *label) {
    const std::vector<Mat2D> errors = r.errors();
    const long nobs = errors[0].rows();
    const Mat2D press_dev = PLS::validation(r, PLS::RESS), mse_dev = PLS::validation(r, PLS::MSE);
    const Mat2D press_host = host_press(errors);
    double worst = 0;
    for (long y = 0; y < press_host.rows(); ++y)
        for (long c = 0; c < press_host.cols(); ++c)
            worst = std::max(worst, std::fabs(press_dev(y, c) - press_host(y, c)) / press_host(y, c));
    const double bound = static_cast<double>(nobs) * std::ldexp(1.0, -52);
    std::printf("%s: nobs %ld, max relative PRESS difference device / host loop %.3e (bound %.3e)\n", label, nobs, worst, bound);
    expect(worst <= bound, "PRESS from the device summary equals the host loop within the summation bound");
    bool mse_ok = true;
    for (long y = 0; y < press_host.rows(); ++y)
        for (long c = 0; c < press_host.cols(); ++c) mse_ok = mse_ok && mse_dev(y, c) == press_dev(y, c) / static_cast<double>(nobs);
    expect(mse_ok, "MSE = RESS / nobs");
    for (float_type alpha : {0.1, 0.01, 0.5}) {
        const Colsz dev = PLS::optimal_num_components(r, alpha);
        const std::vector<size_t> host = host_pick(errors, press_host, alpha);
        bool same = static_cast<size_t>(dev.size()) == host.size();
        for (size_t y = 0; same && y < host.size(); ++y) same = dev[static_cast<long>(y)] == host[y];
        std::printf("%s: alpha %.2f picks device %zu, host %zu (first response)\n", label, alpha, dev[0], host[0]);
        expect(same, "optimal_num_components from the device summary equals the host wilcoxon() loop");
    }
}

int correctness(const char *xfile, const char *yfile) {
    const Mat2D X = PLS::colwise_z_scores(PLS::read_matrix_file(xfile));
    const Mat2D Y = PLS::colwise_z_scores(PLS::read_matrix_file(yfile));
    const size_t A = 10;
    PLS::Model m(X, Y, PLS::KERNEL_TYPE1, A);
    check_residual(m.cv_LOO(), "cv_LOO");
    std::mt19937 rng(12345);
    check_residual(m.cv_LSO(0.3, 200, rng), "cv_LSO(0.3, 200)");
    // cv_NEW_DATA (one X R pass) against one residuals() call per component count
    const PLS::Residual nd = m.cv_NEW_DATA(X, Y);
    double ymax = 0, worst = 0;
    for (long j = 0; j < Y.cols(); ++j)
        for (long i = 0; i < Y.rows(); ++i) ymax = std::max(ymax, std::fabs(Y(i, j)));
    for (size_t nc = 1; nc <= A; ++nc) {
        const Mat2D res = m.residuals(X, Y, nc);
        for (long j = 0; j < res.cols(); ++j)
            for (long i = 0; i < res.rows(); ++i)
                worst = std::max(worst, std::fabs(res(i, j) - nd.errors()[static_cast<size_t>(j)](i, static_cast<long>(nc) - 1)));
    }
    std::printf("cv_NEW_DATA: max |one pass - residuals(c)| = %.3e, max |Y| = %.3e\n", worst, ymax);
    expect(worst <= 1e-12 * ymax, "cv_NEW_DATA equals A separate residuals() calls within 1e-12 max|Y|");
    expect(nd.method() == "NEW DATA", "label");
    check_residual(nd, "cv_NEW_DATA");
    std::printf(failures ? "validation_summary: %d FAILED\n" : "validation_summary: ok\n", failures);
    return failures ? 1 : 0;
}

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

#define HIP_OK(call)                                                                   \
    do {                                                                               \
        if ((call) != hipSuccess) { std::printf("FAIL %s\n", #call); return 2; }      \
    } while (0)

int measure(long M, long nobs, long A, int reps) {
    // the generator of tests/test_validation_ref.py (another random stream: only the shape of the data matters here)
    std::mt19937_64 rng(7);
    std::normal_distribution<double> nd;
    std::vector<double> e(static_cast<size_t>(M * nobs * A)), base(static_cast<size_t>(nobs));
    for (long m = 0; m < M; ++m) {
        for (double &b : base) b = nd(rng);
        const long cs = std::max(0L, 2 * A / 3 - m % 3);
        for (long c = 0; c < A; ++c) {
            const long k = std::labs(c - cs);
            const double g = c < cs ? (k <= 2 ? 0.6 * k : 4.0 * k) / std::sqrt(static_cast<double>(nobs)) : 0.05 * k;
            double *col = e.data() + (m * A + c) * nobs;
            for (long i = 0; i < nobs; ++i) col[i] = (1.0 + g) * base[static_cast<size_t>(i)] + 0.3 * nd(rng);
        }
    }
    pls_hip_handle h = nullptr;
    if (pls_hip_create(&h, 0, nullptr) != PLS_HIP_OK) { std::printf("FAIL pls_hip_create\n"); return 2; }
    double *dE = nullptr, *dP = nullptr, *dD = nullptr, *dW = nullptr;
    int64_t *dR = nullptr;
    const size_t bytes = e.size() * 8, ma = static_cast<size_t>(M * A) * 8;
    HIP_OK(hipMalloc(reinterpret_cast<void **>(&dE), bytes));
    HIP_OK(hipMalloc(reinterpret_cast<void **>(&dP), ma));
    HIP_OK(hipMalloc(reinterpret_cast<void **>(&dD), ma));
    HIP_OK(hipMalloc(reinterpret_cast<void **>(&dW), ma));
    HIP_OK(hipMalloc(reinterpret_cast<void **>(&dR), static_cast<size_t>(M) * 8));
    HIP_OK(hipMemcpy(dE, e.data(), bytes, hipMemcpyHostToDevice));
    auto call = [&]() { return pls_hip_validation(h, dE, nobs, A, M, PLS_HIP_MEM_DEVICE, dP, dD, dW, dR); };
    for (int i = 0; i < 3; ++i)
        if (call() != PLS_HIP_OK) { std::printf("FAIL pls_hip_validation: %s\n", pls_hip_last_error(h)); return 2; }
    pls_hip_synchronize(h);
    pls_hip_set_option(h, PLS_HIP_OPT_PROFILE, 2);
    pls_hip_timing t;
    pls_hip_get_timing(h, &t);
    std::printf("@measure M %ld nobs %ld A %ld reps %d\n", M, nobs, A, reps);
    for (int i = 0; i < reps; ++i) {
        const double w0 = now();
        call();
        pls_hip_get_timing(h, &t);  // synchronises
        const double wall = now() - w0;
        std::printf("@device rep %d press_ms %.4f press_bytes %lld sort_ms %.4f sort_launches %lld wall_ms %.4f\n", i,
                    t.fam_ms[PLS_HIP_FAM_XTY], static_cast<long long>(t.fam_bytes[PLS_HIP_FAM_XTY]), t.fam_ms[PLS_HIP_FAM_SMALL],
                    static_cast<long long>(t.fam_launches[PLS_HIP_FAM_SMALL]), wall * 1e3);
    }
    pls_hip_set_option(h, PLS_HIP_OPT_PROFILE, 0);
    std::vector<double> probw(static_cast<size_t>(M * A));
    std::vector<int64_t> ref(static_cast<size_t>(M));
    HIP_OK(hipMemcpy(probw.data(), dW, ma, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(ref.data(), dR, static_cast<size_t>(M) * 8, hipMemcpyDeviceToHost));
    // the host path: download, then the loops
    const int hreps = nobs > 100000 ? 3 : 20;
    for (int i = 0; i < hreps; ++i) {
        std::vector<double> back(e.size());
        const double t0 = now();
        HIP_OK(hipMemcpy(back.data(), dE, bytes, hipMemcpyDeviceToHost));
        const double t1 = now();
        std::vector<Mat2D> errors(static_cast<size_t>(M), Mat2D::Zero(nobs, A));
        for (long m = 0; m < M; ++m) std::memcpy(errors[static_cast<size_t>(m)].data(), back.data() + m * nobs * A, static_cast<size_t>(nobs * A) * 8);
        const double t2 = now();
        const Mat2D press = host_press(errors);
        const double t3 = now();
        const std::vector<size_t> best = host_pick(errors, press, 0.1);
        const double t4 = now();
        bool same = true;
        for (long m = 0; m < M; ++m) {
            long pick = ref[static_cast<size_t>(m)];
            for (long alt = 0; alt < ref[static_cast<size_t>(m)]; ++alt)
                if (probw[static_cast<size_t>(m + alt * M)] > 0.1) { pick = alt; break; }
            same = same && best[static_cast<size_t>(m)] == static_cast<size_t>(pick) + 1;
        }
        if (i == 0 && !same) {  // beyond the wrap: the same early-exit loop with the unwrapped variance
            bool same2 = true;
            for (long m = 0; m < M; ++m) {
                const long r = ref[static_cast<size_t>(m)];
                long pick_h = r, pick_d = r;
                for (long alt = 0; alt < r; ++alt)
                    if (wilcoxon_unwrapped(errors[static_cast<size_t>(m)].col(r), errors[static_cast<size_t>(m)].col(alt)) > 0.1) { pick_h = alt; break; }
                for (long alt = 0; alt < r; ++alt)
                    if (probw[static_cast<size_t>(m + alt * M)] > 0.1) { pick_d = alt; break; }
                same2 = same2 && pick_h == pick_d;
            }
            std::printf("@host picks with n(n+1)(2n+1) in fp64 equal the device's: %d\n", same2 ? 1 : 0);
        }
        std::printf("@host rep %d download_ms %.3f unpack_ms %.3f press_ms %.3f wilcoxon_ms %.3f picks_equal %d\n", i, (t1 - t0) * 1e3,
                    (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3, same ? 1 : 0);
    }
    hipFree(dE); hipFree(dP); hipFree(dD); hipFree(dW); hipFree(dR);
    pls_hip_destroy(h);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc >= 5 && std::strcmp(argv[1], "--measure") == 0)
        return measure(std::atol(argv[2]), std::atol(argv[3]), std::atol(argv[4]), argc > 5 ? std::atoi(argv[5]) : 20);
    if (argc != 3) return 100;
    return correctness(argv[1], argv[2]);
}
