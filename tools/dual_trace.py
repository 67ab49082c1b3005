"""Which kernels the multi-item calls of the sample-space plan launch, for comparing two builds of the library
(profiles/dual_round).
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/dual_trace.py     the calls of
        tests/test_gpu_dual_launches.py (cv_folds, fit_batch, fit_resampled, cv_press_batch under ALGO_DUAL, three rounds with
        a partial last one, M = 1 and 3, fp64 and fp32), each once
    python tools/dual_trace.py --list DIR > listing.txt     the trace as lines of: kernel, grid (workgroups), workgroup,
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
        if "synth_" in name or "at::" in name:  # (the inputs: the library's generators, torch's copies)
            continue
        wg = [int(r["Workgroup_Size_" + a]) for a in "XYZ"]
        grid = [int(r["Grid_Size_" + a]) // w for a, w in zip("XYZ", wg)]
        print(f"{name}  grid {grid[0]} x {grid[1]}  workgroup {wg[0]}  lds {r['LDS_Block_Size']}")


def calls():
    import torch, pls_amd
    from conftest import handle_with_env
    from test_gpu_dual_launches import CAP, CASES, ROUND_ENV, run_call
    torch.cuda.set_device(0)
    for kind, M, dt in CASES:
        with handle_with_env(**{ROUND_ENV[kind]: CAP}) as h:
            h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
            run_call(h, kind, M, dt)


if __name__ == "__main__":
    listing(sys.argv[2]) if sys.argv[1:2] == ["--list"] else calls()
