// turnaround_probe -- can consecutive in-place sweeps of a matrix far larger than the 256 MiB Infinity Cache hand their
// turning point over on-die?  Sweep a walks the tiles in one direction, sweep a + 1 in the other, so the first S bytes of
// a sweep are the last S bytes the sweep before it stored.  The bulk keeps the nt (streaming) policy of the fused pass;
// the first E and the last E rounds of a sweep (one round = grid x tile = 32 MB) take a policy of their own for loads and
// for stores.  Questions: does nt bulk traffic leave default-policy lines of the edge resident, and what does an nt or
// a default store do to a dirty resident line?
// Access shape of the headline pass: 128 KB contiguous tiles, 512 lanes x 16 B x 16 loads through one buffer descriptor
// per tile, one workgroup per CU, positions dealt cyclically; position q is tile q (ascending) or ntiles - 1 - q.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -o turnaround_probe turnaround_probe.hip
// Run:   turnaround_probe [buffer MiB = 4096] [pairs of sweeps timed = 8]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef long long i64;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)

constexpr int BUF_WORD3 = 0x00020000;
constexpr int NTH = 512, CPT = 16;
constexpr int TILE_BYTES = NTH * 16 * CPT;  // 128 KB
constexpr int GSTEP = NTH * 16;
// policy of a tile: bit 1 = nt loads, bit 0 = nt stores (0 = default policy on both)
constexpr int POL_NT = 3;

template <bool LDNT, bool STNT, bool WRITE>
__device__ __forceinline__ void tile_body(char *p, uint32_t off, double a, double b, double &acc) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(p, (short)0, TILE_BYTES, BUF_WORD3);
    u32x4 x[CPT];
#pragma unroll
    for (int j = 0; j < CPT; ++j) x[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, off, j * GSTEP, LDNT ? 2 : 0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        double d[2];
        __builtin_memcpy(d, &x[j], 16);
        d[0] = fma(d[0], a, b);
        d[1] = fma(d[1], a, b);
        if (WRITE) {
            __builtin_memcpy(&x[j], d, 16);
            __builtin_amdgcn_raw_buffer_store_b128(x[j], rs, off, j * GSTEP, STNT ? 2 : 0);
        } else {
            acc += d[0] * d[1];
        }
    }
}

// E: edge length in rounds; lead / trail: policy of the first / last E rounds of the walk; a buffer of fewer than two
// edges is all edge and takes `lead` throughout
template <bool WRITE>
__global__ __launch_bounds__(NTH) void sweep(char *X, i64 ntiles, int reverse, int E, int lead, int trail, double a, double b,
                                             double *sink) {
    const uint32_t off = threadIdx.x * 16u;
    const i64 nrounds = (ntiles + gridDim.x - 1) / gridDim.x;
    const bool alledge = 2 * (i64)E >= nrounds;
    double acc = 0.0;
    i64 round = 0;
    for (i64 pos = blockIdx.x; pos < ntiles; pos += gridDim.x, ++round) {
        const i64 tile = reverse ? ntiles - 1 - pos : pos;
        char *p = X + tile * TILE_BYTES;
        const int pol = (E == 0) ? POL_NT : (alledge || round < E) ? lead : (round >= nrounds - E ? trail : POL_NT);
        if (pol == POL_NT) tile_body<true, true, WRITE>(p, off, a, b, acc);
        else if (pol == 0) tile_body<false, false, WRITE>(p, off, a, b, acc);
        else if (pol == 2) tile_body<true, false, WRITE>(p, off, a, b, acc);
        else tile_body<false, true, WRITE>(p, off, a, b, acc);
    }
    if (acc == 1.2345e300) sink[0] = acc;
}

struct Case {
    const char *name;
    bool write, alternate;
    int lead, trail;  // policies of the edges
    bool all;         // the whole sweep is edge (E = rounds): the default policy everywhere
};

int main(int argc, char **argv) {
    const i64 mib = argc > 1 ? atoll(argv[1]) : 4096;
    const int pairs = argc > 2 ? atoi(argv[2]) : 8;
    const i64 bytes = mib << 20;
    const i64 ntiles = bytes / TILE_BYTES;
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int grid = prop.multiProcessorCount;
    const double round_mb = (double)grid * TILE_BYTES / 1e6;
    char *X;
    double *sink;
    CK(hipMalloc(&X, bytes));
    CK(hipMalloc(&sink, 8));
    CK(hipMemset(X, 0, bytes));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    printf("# buffer %lld MiB = %lld tiles of %d KB, grid %d (one round = %.1f MB), %d timed pairs of sweeps, median of 5\n",
           mib, ntiles, TILE_BYTES / 1024, grid, round_mb, pairs);

    auto run = [&](const Case &c, int E) {
        auto one = [&](int s) {
            const int rev = c.alternate ? (s & 1) : 0;
            if (c.write) hipLaunchKernelGGL(sweep<true>, dim3(grid), dim3(NTH), 0, 0, X, ntiles, rev, E, c.lead, c.trail, 1.0, 0.0, sink);
            else hipLaunchKernelGGL(sweep<false>, dim3(grid), dim3(NTH), 0, 0, X, ntiles, rev, E, c.lead, c.trail, 1.0, 0.0, sink);
            CK(hipGetLastError());
        };
        std::vector<double> ts;
        for (int rep = 0; rep < 5; ++rep) {
            one(0); one(1);
            CK(hipEventRecord(e0));
            for (int s = 0; s < 2 * pairs; ++s) one(s);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            ts.push_back(ms / (2.0 * pairs));
        }
        std::sort(ts.begin(), ts.end());
        return ts[2];  // ms per sweep
    };

    const Case cases[] = {
        {"rw  lead ld=def st=def | trail ld=nt  st=def", true, true, 0, 2, false},
        {"rw  lead ld=def st=nt  | trail ld=nt  st=def", true, true, 1, 2, false},
        {"rw  lead ld=def st=def | trail ld=def st=def", true, true, 0, 0, false},
        {"rw  lead ld=nt  st=def | trail ld=nt  st=def", true, true, 2, 2, false},
        {"ro  lead ld=def        | trail ld=def       ", false, true, 0, 0, false},
    };
    const int edges[] = {0, 2, 4, 6, 7};
    for (int w = 1; w >= 0; --w) {
        const Case asc = {"ascending, all nt", w == 1, false, POL_NT, POL_NT, false};
        const double base = run(asc, 0);
        const double vol = (w ? 2.0 : 1.0) * bytes;
        printf("%s ascending, all nt (the library today):          %8.4f ms/sweep  %6.0f GB/s\n", w ? "rw" : "ro", base, vol / base / 1e6);
        for (const Case &c : cases) {
            if (c.write != (w == 1)) continue;
            for (int E : edges) {
                const double t = run(c, E);
                printf("%s  S = %3.0f MB (E = %d): %8.4f ms/sweep  %6.0f GB/s  saving %+7.1f us  %+6.2f %%\n", c.name, E * round_mb, E, t,
                       vol / t / 1e6, (base - t) * 1e3, 100.0 * (base - t) / base);
            }
        }
        // the default policy on every access, ascending and alternating (what profiles/last_pass/serpentine_ab.txt measured in the library)
        const Case dasc = {"", w == 1, false, 0, 0, true}, dalt = {"", w == 1, true, 0, 0, true};
        const int Eall = (int)((ntiles + grid - 1) / grid);
        const double ta = run(dasc, Eall), tb = run(dalt, Eall);
        printf("%s default policy everywhere: ascending %8.4f ms/sweep, alternating %8.4f ms/sweep (%+.1f us)\n", w ? "rw" : "ro", ta, tb, (ta - tb) * 1e3);
        const double base2 = run(asc, 0);
        printf("%s ascending, all nt, again (drift check):           %8.4f ms/sweep\n", w ? "rw" : "ro", base2);
    }
    return 0;
}
