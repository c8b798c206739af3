"""The case table of the team ensemble-fit tests (tests/test_gpu_dyn_fit_team.py, tests/test_dyn_fit_team_cpu.py) and its data
recipe: NumPy only, so the CPU test reads the table the GPU worker runs."""
import numpy as np

from tests._dyn_check import rand_theta, rand_tr

LR, WD = 1e-3, 1e-3
GRAD_FLOOR = 3e-7             # (tests/_dyn_ensemble_cases.py)
ILL_SHARE = 2.8e-2            # the most a case may leave out of the parameter comparison

# name, sizes, batch, act (0 ReLU, 1 tanh), target mode, K, the team's G (0: not served -- route 1, bit for bit)
CASES = [
    ("w64_b16", [13, 64, 64, 11], 16, 1, 2, 3, 2),            # one 32-unit tile a slice, d_in % 8 != 0, d_out padded to 32
    ("w128_b33", [13, 128, 128, 11], 33, 1, 2, 3, 4),         # Bp 64 with 31 padded sample columns
    ("w128_256_b64", [13, 128, 256, 11], 64, 0, 2, 3, 4),     # slices of 32 and 64 units
    ("w192_64_b32", [24, 192, 64, 5], 32, 0, 1, 3, 2),        # slices of 96 and 32 units, target mode 1
    ("max_b64", [128, 256, 256, 64], 64, 0, 2, 3, 4),         # every limit at once: 139 KiB of tiles
    ("k1_b64", [13, 128, 128, 11], 64, 0, 2, 1, 4),           # a single team
]
# name, sizes, batch, MJX_DYN_FIT_TEAM: the _team entry IS mjx_dyn_fit_ensemble
FALL_THROUGH = [("w96", [13, 96, 96, 11], 16, None), ("switch_off", [13, 128, 128, 11], 16, "0"), ("b65", [13, 64, 64, 11], 65, None)]


def member_data(name, sizes, batch, k):
    """member k of a case on N = 5 batch + 7 rows -> (theta, transforms, x, y, row indices of three epochs of five steps)"""
    rng = np.random.RandomState(900 + 31 * k + len(name))
    din, dout, N = sizes[0], sizes[-1], 5 * batch + 7
    x = rng.randn(N, din).astype(np.float32)
    y = (x[:, :dout] * 0.8 + 0.3 * rng.randn(N, dout)).astype(np.float32)
    idx = np.concatenate([rng.permutation(N)[:5 * batch] for _ in range(3)])
    return rand_theta(rng, sizes), rand_tr(rng, din, dout), x, y, idx


def members(name, sizes, batch, K):
    d = [member_data(name, sizes, batch, k) for k in range(K)]
    return tuple(np.stack([m[q] for m in d]) for q in range(5))        # th, tr, x, y, idx
