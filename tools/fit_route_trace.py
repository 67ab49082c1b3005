"""Which kernels a fit launches and the bits it computes, for comparing two builds of the library (profiles/fit_route).
    python tools/fit_route_trace.py [bits.txt]     one device-memory fit per row of FITS under a fixed seed; per row one SHA-256
        over the bytes of W, P, Q, R, B and T
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/fit_route_trace.py     the same run, traced
    python tools/fit_route_trace.py --list DIR > listing.txt     the trace as lines of: kernel, grid (workgroups), workgroup,
        LDS bytes -- in launch order, the kernels of the synthetic inputs and torch's own left out
FITS: the rows of tests/test_fit_route.py whose X is below 500 MB and that one handle can run (no reducer, no upload), one shape
per single-launch route, and two AUTO shapes on either side of the cost model.  PLS_AMD_LIBRARY selects the build."""
import csv, glob, hashlib, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def short(name):
    """a kernel's name with its template arguments, without its parameter list"""
    if not name.endswith(")"):
        return name
    depth = 0
    for i in range(len(name) - 1, -1, -1):
        depth += (name[i] == ")") - (name[i] == "(")
        if depth == 0:
            return name[:i]
    return name


def listing(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        name = re.sub(r"^void ", "", r["Kernel_Name"])
        if "plsk::" not in name or "plsk::synth_" in name:
            continue
        wg = [int(r["Workgroup_Size_" + a]) for a in "XYZ"]
        grid = [int(r["Grid_Size_" + a]) // w for a, w in zip("XYZ", wg)]
        print(f"{short(name)}  grid {grid[0]} x {grid[1]}  workgroup {wg[0]}  lds {r['LDS_Block_Size']}")


def fits():
    from test_fit_route import AUTO, KERNEL, ROWS, fit
    rows = [(name, d) for name, d, _ in ROWS
            if d["N"] * d["K"] * (8 if d["dt"] == "f64" else 4) < 500e6 and not (d["reducer"] or d["pre"] or d["xep"] or d["denied"])]
    # the single-launch routes: one workgroup (1 and 3 responses), one wave, resident (1 and 4 responses), resident X^T X in its
    # row form and its block form
    rows += [("single launch: " + name, fit(N, K, M, A, "f64", algo)) for name, N, K, M, A, algo in
             [("tiny", 130, 120, 1, 9, KERNEL), ("tiny_m", 130, 100, 3, 7, KERNEL), ("micro", 10, 15, 2, 2, KERNEL),
              ("resident", 4001, 416, 1, 6, KERNEL), ("resident_m", 5000, 128, 4, 8, KERNEL),
              ("resident X^T X", 1025, 26, 1, 5, AUTO), ("resident X^T X", 5000, 128, 1, 10, AUTO)]]
    rows += [("AUTO -> GRAM", fit(300000, 64, 1, 12, "f64", AUTO)), ("AUTO -> KERNEL", fit(8192, 1024, 1, 2, "f64", AUTO))]
    return rows


def run(out_path):
    import torch, pls_amd
    h = pls_amd.Handle()
    lines = []
    for name, d in fits():
        N, K, M, A = d["N"], d["K"], d["M"], d["A"]
        dt = torch.float64 if d["dt"] == "f64" else torch.float32
        for opt, key in ((pls_amd.OPT_ALGO, "algo"), (pls_amd.OPT_FUSE, "fuse"), (pls_amd.OPT_WORK_LAYOUT, "layout"), (pls_amd.OPT_DEFER, "defer"),
                         (pls_amd.OPT_FUSED_GRID, "grid")):
            h.set_option(opt, d[key])
        X, Y = h.synth_x(0, N, K, 31, dtype=dt), h.synth_y(0, N, M, 31, dtype=dt)
        if d["ldx"] or d["xmod"]:  # a leading dimension of its own, a base off the 16-byte grid
            ld, off = d["ldx"] or X.stride(1), d["xmod"] // X.element_size()
            flat = torch.zeros(ld * K + 16, dtype=dt, device="cuda")
            Xo = flat[off:off + ld * K].view(K, ld)[:, :N].t()
            Xo.copy_(X)
            X = Xo
            assert X.data_ptr() % 16 == d["xmod"]
        out = h.fit_device(X, Y, A, method=d["method"])
        h.synchronize()
        sha = hashlib.sha256()
        for k in "WPQRBT":
            if out[k] is not None:
                sha.update(out[k].cpu().contiguous().numpy().tobytes())
        lines.append(f"{name}: N={N} K={K} M={M} A={A} {d['dt']} algo={d['algo']} method={d['method']}  {sha.hexdigest()}")
        del X, Y, out
    print("\n".join(lines))
    if out_path:
        open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    listing(sys.argv[2]) if sys.argv[1:2] == ["--list"] else run(sys.argv[1] if len(sys.argv) > 1 else None)
