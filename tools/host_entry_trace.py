"""The bits every entry point with a `mem` argument computes and the kernels it launches, for comparing two builds of the library
(profiles/host_stage).
    python tools/host_entry_trace.py [bits.txt]     every case of tests/test_gpu_host_stage.CASES as a host-memory call and as the
        device-memory call of the staged layout, then MASKS: the optional outputs of x_diagnostics, fit_resampled, fit_batch and
        validation in subsets; per call one SHA-256 over the bytes of every output
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/host_entry_trace.py     the same run, traced
    python tools/host_entry_trace.py --list DIR > listing.txt     the trace as lines of: kernel, grid (workgroups), workgroup,
        LDS bytes -- in launch order, torch's own kernels left out
PLS_AMD_LIBRARY selects the build."""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

MASKS = [("x_diagnostics", w) for w in (("Q",), ("T2",), ("S",), ("ssx",), ("sst",), ("Q", "sst"), ("T2", "S", "ssx"), ())] + \
        [("fit_resampled", w) for w in (("B0",), ("Bmean", "Bm2"), ("Q", "tt"), ("B",), ("B", "B0", "Bm2"))] + \
        [("fit_batch", w) for w in (("B",), ("R", "Q"), ("tt", "ssy"))] + \
        [("validation", w) for w in (("PRESS",), ("PRESS", "ref"), ("D",), ("probw", "ref"), ("D", "probw"))]


def run(out_path):
    import torch, pls_amd
    from pls_amd import _lib as L
    from test_gpu_host_stage import CASES, run_case
    torch.cuda.set_device(0)
    plain, sharded = pls_amd.Handle(), pls_amd.Handle()
    cb = L.ALLREDUCE_FN(lambda user, buf, count, stream: 0)  # (one rank: the sum is the identity)
    L.check(L.lib().pls_hip_set_reducer(sharded.h, cb, None, 0, 1), sharded.h)
    calls = [(e, dt, N, M, None) for e, dt, N, M in CASES]
    calls += [(e, dt, N, 2, w) for e, w in MASKS for dt in ("f64", "f32") for N in (37, 38)]
    lines = []
    for entry, dt, N, M, want in calls:
        h = sharded if entry == "cv_folds_sharded" else plain
        for device in (False, True):
            sha = hashlib.sha256()
            for a in run_case(h, entry, dt, N, M, device, want):
                sha.update(a.tobytes())
            mask = "" if want is None else " want=" + "+".join(want)
            lines.append(f"{entry} {dt} N={N} M={M} {'device' if device else 'host'}{mask}  {sha.hexdigest()}")
    print("\n".join(lines))
    if out_path:
        open(out_path, "w").write("\n".join(lines) + "\n")
    plain.close()
    sharded.close()


if __name__ == "__main__":
    if sys.argv[1:2] == ["--list"]:
        from fit_route_trace import listing
        listing(sys.argv[2])
    else:
        run(sys.argv[1] if len(sys.argv) > 1 else None)
