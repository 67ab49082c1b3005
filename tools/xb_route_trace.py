"""Which kernels X * Bm launches, for comparing two builds of the library (profiles/xb_route).
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/xb_route_trace.py     one pls_hip_xb per row of
        tests/test_gpu_bounds.XB_ROUTES (its layouts and PLS_HIP_XB4) and per shape of the X * B parity tests
    python tools/xb_route_trace.py --list DIR > listing.txt     the trace as lines of: kernel, grid (workgroups), workgroup,
        LDS bytes -- in launch order, the kernels of the synthetic inputs left out
PLS_AMD_LIBRARY selects the build."""
import csv, glob, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def listing(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        name = re.sub(r"^void ", "", r["Kernel_Name"])
        if not re.match(r"(plsk::)?xb_", name):
            continue
        wg = [int(r["Workgroup_Size_" + a]) for a in "XYZ"]
        grid = [int(r["Grid_Size_" + a]) // w for a, w in zip("XYZ", wg)]
        print(f"{name}  grid {grid[0]} x {grid[1]}  workgroup {wg[0]}  lds {r['LDS_Block_Size']}")


def calls():
    import torch, pls_amd
    from pls_amd import _lib as L
    from test_gpu_bounds import XB_ROUTES
    hs = {}

    def handle(xb4):
        if xb4 not in hs:
            if xb4 is not None: os.environ["PLS_HIP_XB4"] = str(xb4)
            hs[xb4] = pls_amd.Handle()
            os.environ.pop("PLS_HIP_XB4", None)
        return hs[xb4]

    def place(rows, cols, dt, layout):  # test_gpu_bounds.Guarded: (view of the flat buffer, ld)
        V = 16 // torch.empty((), dtype=dt).element_size()
        ld = rows if layout == "eigen" else -(-rows // V) * V + V
        off = 1 if layout == "eigen" else 0
        return torch.zeros(ld * cols + V, dtype=dt, device="cuda")[off:], ld

    for N, K, C, dt, xl, ol, xb4 in XB_ROUTES:
        h, tdt = handle(xb4), torch.float64 if dt == "f64" else torch.float32
        code = L.F64 if dt == "f64" else L.F32
        X, ldx = place(N, K, tdt, xl)
        out, ldo = place(N, C, tdt, ol)
        L.check(L.lib().pls_hip_synth_x(h.h, X.data_ptr(), ldx, 0, N, K, 41, code), h.h)
        Bm = torch.ones(K, C, dtype=torch.float64, device="cuda").t().contiguous().t()
        L.check(L.lib().pls_hip_xb(h.h, X.data_ptr(), ldx, N, K, Bm.data_ptr(), K, C, code, L.MEM_DEVICE, out.data_ptr(), ldo), h.h)
        h.synchronize()
        del X, out
    h = handle(None)
    steps = [(9, 7, 2), (1000, 64, 4), (4097, 513, 8), (2048, 512, 1), (777, 33, 3)]
    many = [(64, 4, 9), (1000, 33, 16), (4099, 130, 17), (777, 63, 32), (2048, 257, 33), (300, 1025, 50), (5001, 100, 64), (1030, 37, 49),
            (2049, 515, 200), (130, 70, 65)]
    tall = [(262144 + 37, 70, 20, "f64"), (262144, 64, 5, "f64"), (300000, 33, 19, "f64"), (270001, 130, 32, "f64"), (262144 + 31, 32, 8, "f64"),
            (524288 + 5, 33, 24, "f32"), (524288, 40, 5, "f32"), (600001, 18, 13, "f32"), (131072, 4096, 8, "f32"), (131072 + 3, 1030, 20, "f64"),
            (262144, 1024, 32, "f64"), (40001, 200, 19, "f64"), (3001, 3000, 7, "f64"), (70000, 130, 24, "f32"), (16388, 2052, 12, "f32"),
            (65536 + 33, 640, 5, "f64"), (20000, 2000, 20, "f32"), (8200, 1500, 9, "f64"), (16390, 700, 17, "f32"), (2000, 20000, 20, "f64"),
            (512, 50000, 8, "f32"), (1001, 9001, 5, "f64"), (130, 70000, 23, "f32"), (64, 140000, 32, "f64")]
    shapes = [(N, K, C, "f64", u) for N, K, C in steps for u in (False, True)]
    shapes += [(N, K, C, dt, False) for dt in ("f32", "f64") for N, K, C in many] + [s + (False,) for s in tall]
    for N, K, C, dt, unaligned in shapes:
        X = h.synth_x(0, N, K, 23, dtype=torch.float64 if dt == "f64" else torch.float32)
        if unaligned:  # test_steps_xty_xb_deflate: an odd base pointer and leading dimension
            big = torch.empty((K, N + 3), dtype=X.dtype, device="cuda")
            Xo = big[:, 1:N + 1].t()
            Xo.copy_(X)
            X = Xo
        h.xb(X, torch.ones(K, C, dtype=torch.float64, device="cuda"))
        h.synchronize()
        del X


if __name__ == "__main__":
    listing(sys.argv[2]) if sys.argv[1:2] == ["--list"] else calls()
