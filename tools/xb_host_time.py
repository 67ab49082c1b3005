"""host-side time of one pls_hip_xb enqueue (one column, a small matrix: the launch path dominates)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, pls_amd
h = pls_amd.Handle()
for N, K, C in ((4096, 64, 1), (4096, 64, 3), (262144 + 5, 128, 3), (2000, 5000, 21)):
    X = h.synth_x(0, N, K, 5)
    B = pls_amd.as_colmajor(torch.randn(K, C, dtype=torch.float64, device="cuda"))
    for _ in range(50): h.xb(X, B)
    h.synchronize()
    best = 1e9
    for rep in range(12):
        n = 300
        t0 = time.perf_counter()
        for _ in range(n): h.xb(X, B)
        dt = (time.perf_counter() - t0) / n
        h.synchronize()
        best = min(best, dt)
    print(f"host enqueue of pls_hip_xb (python wrapper included) N={N} K={K} C={C}: best of 12 x 300: {best*1e6:.2f} us", flush=True)
