"""Worker of tests/test_gpu_gemm_chain.py: runs a list of cases through the layer-wise path with whatever MJX_* switches the
parent set in the environment (most are read once per process) and writes one .npz of device results per case.

    python _gemm_chain_worker.py <spec.json> <out_dir>

spec.json: {"kind": "cases" | "stale", "cases": [{...}, ...]}.  The inputs are rebuilt from the case's seed by chain_inputs(),
which the parent calls too (for the fp64 oracle)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import npg_oracle as O  # noqa: E402
from tests._dispatch_matrix_worker import _engine, _pack, head_inputs  # noqa: E402


def chain_inputs(n, m, hid, N, seed):
    """head_inputs() (every action with its own log_std and output transform, non-identity input transforms, on-policy actions,
    an old network th2 != th, a direction v) plus tr2: the new network's transforms of the general Hessian, all four vectors
    moved away from tr"""
    inp = head_inputs(n, m, hid, N, seed)
    rng = np.random.RandomState(seed + 1)
    tr = inp["tr"]
    tr2 = O.Transforms(n, m, tr.in_shift + 0.05 * rng.randn(n), tr.in_scale * (1 + 0.05 * rng.rand(n)),
                       tr.out_shift + 0.05 * rng.randn(m), tr.out_scale * (1 + 0.05 * rng.rand(m)))
    inp.update(tr2=tr2, pk2=_pack(tr2))
    return inp


def products(eng, inp):
    """K1 with an explicit old network, K3 at the same binding, K2 at old == new, the general Hessian (old != new, own transforms)"""
    import torch
    th, th2, pk, pk2 = inp["th"], inp["th2"], inp["pk"], inp["pk2"]
    out = {}
    eng.set_policy(th2, th, pk, pk)
    eng.set_batch(inp["obs"], inp["act"], inp["adv"])
    out["g2"] = eng.surr_vpg()[0].cpu().numpy().copy()
    out["s"], out["kl"] = eng.eval_surr_kl()
    v = torch.from_numpy(inp["v"]).to(eng.device)
    eng.set_policy(th, th, pk, pk)
    out["hv"] = eng.fvp(v).cpu().numpy().copy()
    eng.set_policy(th2, th, pk2, pk)
    out["gh"] = eng.fvp(v).cpu().numpy().copy()
    return out


def policy_forward(eng, inp):
    """the policy's means through the C ABI's mjx_policy_forward (the layer-wise forward chain on its own)"""
    import torch
    from mjrl_amd._lib import check, ptr
    obs = eng.to_device_f32(inp["obs"])
    th = torch.from_numpy(inp["th"]).to(eng.device)
    pk = torch.from_numpy(inp["pk"]).to(eng.device)
    mu = torch.empty((obs.shape[0], eng.m), dtype=torch.float32, device=eng.device)
    check(eng.lib.mjx_policy_forward(eng.ctx, ptr(obs), obs.shape[0], ptr(th), ptr(pk), ptr(mu), eng.stream()))
    return mu.cpu().numpy().copy()


def run_case(c):
    n, m, hid = c["n"], c["m"], tuple(c["hid"])
    inp = chain_inputs(n, m, hid, c["N"], c["seed"])
    eng = _engine(n, m, hid)
    out = {"mu": policy_forward(eng, inp)}
    out.update(products(eng, inp))
    eng.close()
    return out


def run_stale(c):
    """the same small batch through a fresh engine and through one that ran a larger batch first (whose rows stay in the
    padding rows of the workspace); both engines live at once, so neither reuses the other's memory"""
    n, m, hid = c["n"], c["m"], tuple(c["hid"])
    small = chain_inputs(n, m, hid, c["N"], c["seed"])
    big = chain_inputs(n, m, hid, c["N_big"], c["seed"] + 7)
    big.update({k: small[k] for k in ("th", "th2", "pk", "pk2", "v")})      # (the same networks: only the rows differ)
    fresh, used = _engine(n, m, hid), _engine(n, m, hid)
    out = {"fresh_" + k: x for k, x in products(fresh, small).items()}
    products(used, big)
    out.update({"used_" + k: x for k, x in products(used, small).items()})
    fresh.close()
    used.close()
    return out


def main():
    spec_path, out_dir = sys.argv[1], sys.argv[2]
    with open(spec_path) as f:
        spec = json.load(f)
    run = run_case if spec["kind"] == "cases" else run_stale
    for c in spec["cases"]:
        np.savez(os.path.join(out_dir, c["name"] + ".npz"), **run(c))


if __name__ == "__main__":
    main()
