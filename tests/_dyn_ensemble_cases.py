"""The case table of the ensemble-fit tests (tests/test_gpu_dynamics_ensemble.py, tests/test_dynamics_ensemble_cpu.py) and
its data recipe: NumPy only, so the CPU tests read the same table the GPU worker runs."""
import numpy as np

from tests._dyn_check import rand_theta, rand_tr

K, NF, LR, WD = 4, 400, 1e-3, 1e-5
GRAD_FLOOR = 3e-7             # parameters whose first fp64 gradient is below this are ill-conditioned for any fp32 Adam

# name, sizes, batch, act (0 ReLU, 1 tanh), target mode: all on route 1
CASES = [
    ("w256_b16", [13, 256, 256, 11], 16, 0, 2),
    ("w256_b64", [13, 256, 256, 11], 64, 0, 2),
    ("pm_b16", [8, 256, 256, 6], 16, 0, 2),
    ("w32_b33", [5, 32, 32, 3], 33, 0, 2),
    ("h64_96_tanh", [10, 64, 96, 8], 32, 1, 1),
    ("din128_dout64", [128, 128, 64, 64], 64, 0, 2),
    ("w64_b32", [10, 64, 64, 8], 32, 0, 2),
]
# every served limit at once: the gathered inputs no longer fit in LDS beside the activations and live in scratch.  Kept out
# of the matrix above (its own keys), so the matrix's ill-conditioned share stays the one its recipe gives.
XSCR_CASE = ("max_b64", [128, 256, 256, 64], 64, 0, 2)
# name, sizes, batch, act, target mode, MJX_DYN_FIT_ENS: route 0, bit for bit K mjx_dyn_fit_adam calls
ROUTE0 = [
    ("w288", [13, 288, 288, 11], 16, 0, 2, None),
    ("hidden3", [10, 64, 64, 64, 8], 32, 0, 2, None),
    ("reward", [24, 100, 100, 1], 32, 0, 0, None),
    ("b65", [10, 64, 64, 8], 65, 0, 2, None),
    ("w64_b32", [10, 64, 64, 8], 32, 0, 2, "0"),
]


def member_data(name, sizes, batch, k, epochs=12):
    """member k of a case: fit_data of tests/_dynamics_matrix_worker.py with seed 500 + 17 k + len(name)
    -> (theta, transforms, x, y, row indices of `epochs` epochs)"""
    rng = np.random.RandomState(500 + 17 * k + len(name))
    din, dout = sizes[0], sizes[-1]
    th = rand_theta(rng, sizes)
    tr = rand_tr(rng, din, dout)
    xf = rng.randn(NF, din).astype(np.float32)
    yf = (xf[:, :dout] * 0.8 + 0.3 * rng.randn(NF, dout)).astype(np.float32) if dout <= din else rng.randn(NF, dout).astype(np.float32)
    idx = np.concatenate([rng.permutation(NF)[:(NF // batch) * batch] for _ in range(epochs)])
    return th, tr, xf, yf, idx
