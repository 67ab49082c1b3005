"""What the multi-item calls of the sample-space plan enqueue: per family the number of bracketed launches and the bytes they
declare (Handle.timing() at profile level 2), for cv_folds, fit_batch, fit_resampled and cv_press_batch under ALGO_DUAL with
three rounds, the last one partial.  The four plans share one round driver (pls_amd/csrc/dual_round.hpp); RECORDED holds the
counters of the commit before they did, when each plan carried its own loop -- exact, these are counters and not times.
    python tests/test_gpu_dual_launches.py      prints the table of the library in use (PLS_AMD_LIBRARY selects the build)"""
import numpy as np
import pytest

from conftest import handle_with_env

pytestmark = pytest.mark.gpu

N, K, A, TS, CAP = 37, 300, 4, 5, 3
ITEMS, NREP = 7, 6  # three rounds at CAP: 3 + 3 + 1; the unit-weight fit of fit_resampled leads its NREP replicates
KINDS = ("cv_folds", "fit_batch", "fit_resampled", "cv_press_batch")
CASES = [(kind, M, dt) for kind in KINDS for M in (1, 3) for dt in ("f64", "f32")]
ROUND_ENV = {"cv_folds": "PLS_HIP_DUALCV_ROUND", "fit_batch": "PLS_HIP_DUALBATCH_ROUND", "fit_resampled": "PLS_HIP_RESAMPLE_ROUND",
             "cv_press_batch": "PLS_HIP_DUALCVB_ROUND"}

# (kind, M, dtype) -> {family: (launches, bytes)}, the families that launched anything
RECORDED = {
    ('cv_folds', 1, 'f64'): {'xty': (1, 99752), 'small': (28, 225816)},
    ('cv_folds', 1, 'f32'): {'xty': (1, 55352), 'small': (28, 225668)},
    ('cv_folds', 3, 'f64'): {'xty': (1, 99752), 'small': (28, 318728)},
    ('cv_folds', 3, 'f32'): {'xty': (1, 55352), 'small': (28, 318284)},
    ('fit_batch', 1, 'f64'): {'xty': (7, 726912), 'small': (30, 242360)},
    ('fit_batch', 1, 'f32'): {'xty': (7, 416112), 'small': (30, 241324)},
    ('fit_batch', 3, 'f64'): {'xty': (7, 764656), 'small': (30, 338120)},
    ('fit_batch', 3, 'f32'): {'xty': (7, 453856), 'small': (30, 335012)},
    ('fit_resampled', 1, 'f64'): {'xty': (5, 473824), 'small': (35, 330216)},
    ('fit_resampled', 1, 'f32'): {'xty': (5, 251824), 'small': (35, 330068)},
    ('fit_resampled', 3, 'f64'): {'xty': (5, 511568), 'small': (35, 572680)},
    ('fit_resampled', 3, 'f32'): {'xty': (5, 289568), 'small': (35, 572236)},
    ('cv_press_batch', 1, 'f64'): {'xty': (1, 99752), 'small': (31, 226304)},
    ('cv_press_batch', 1, 'f32'): {'xty': (1, 55352), 'small': (31, 225128)},
    ('cv_press_batch', 3, 'f64'): {'xty': (1, 99752), 'small': (31, 320192)},
    ('cv_press_batch', 3, 'f32'): {'xty': (1, 55352), 'small': (31, 316664)},
}


def run_call(h, kind, M, dt):
    """one call of `kind` on handle h (ALGO_DUAL set, its round capped at CAP): ITEMS items, on synthetic device data"""
    import torch
    import pls_amd
    tdt = torch.float64 if dt == "f64" else torch.float32
    X = h.synth_x(0, N, K, 11, dtype=tdt)
    idx = np.random.default_rng(3).permutation(N)[:ITEMS * TS].reshape(ITEMS, TS)
    if kind == "cv_folds":
        h.cv_folds(X, h.synth_y(0, N, M, 11, dtype=tdt), A, idx)
    elif kind == "fit_batch":
        h.fit_batch(X, h.synth_y(0, N, ITEMS * M, 11, dtype=tdt), M, A, want=("R", "Q", "tt", "B", "ssy"))
    elif kind == "fit_resampled":
        W = pls_amd.as_colmajor(torch.from_numpy(np.random.default_rng(5).integers(0, 3, (N, NREP)).astype(np.float64)).cuda())
        h.fit_resampled(X, h.synth_y(0, N, M, 11, dtype=tdt), A, W, want=("B", "Bmean"))
    else:
        h.cv_press_batch(X, h.synth_y(0, N, M, 11, dtype=tdt), M, A, idx, want=("PRESS", "ssy"))
    h.synchronize()


def counters(kind, M, dt):
    import pls_amd
    with handle_with_env(**{ROUND_ENV[kind]: CAP}) as h:
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
        run_call(h, kind, M, dt)  # (sizes every workspace; the synthetic inputs are not bracketed)
        h.set_option(pls_amd.OPT_PROFILE, 2)
        h.timing()
        run_call(h, kind, M, dt)
        t = h.timing()
    return {f: (t["launches"][f], t["bytes"][f]) for f in t["launches"] if t["launches"][f]}


@pytest.mark.parametrize("kind,M,dt", CASES)
def test_launches_and_bytes_are_the_recorded_ones(handle, kind, M, dt):
    got = counters(kind, M, dt)
    print(f"{(kind, M, dt)}: {got}")
    assert got == RECORDED[(kind, M, dt)]


if __name__ == "__main__":
    import torch
    torch.cuda.set_device(0)
    print("RECORDED = {")
    for case in CASES:
        print(f"    {case!r}: {counters(*case)!r},")
    print("}")
